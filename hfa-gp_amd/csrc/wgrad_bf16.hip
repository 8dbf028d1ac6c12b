// Weight gradient of the 3x3 modulated conv on v_mfma_f32_32x32x16_bf16 with split operands (gfx950):
//     dW[tap][ci][co] = sum_{b, pos} (x s)[b][pos + tap][ci] * g[b][pos][co]
// Same decomposition as wgrad.hip (M = ci, N = co, K = positions; a block owns a 64 x 64 (ci, co) tile for all nine
// taps and walks 4 x 16 position tiles; split-K slabs + wgrad_sum_final_kernel), but the products are BF16X3: both
// operands are split into hi + lo bf16 parts (a gradient needs fp32's exponent range, which bf16 keeps) and a
// product is hi.hi + lo.hi + hi.lo accumulated in fp32 — 3 MFMAs of the 16x faster pipe instead of 8 fp32 MFMAs
// per 16 positions.
//
// A 16-bit MFMA operand is 8 K-CONTIGUOUS values per lane, and K = positions here, so the patches are TRANSPOSED on
// their way into LDS: x as [part][ci][patch position], g as [part][co][tile position] (a staging thread loads 4
// neighbouring positions x 4 channels and writes, per channel and part, one 8-byte run of 4 positions).  One MFMA
// K step = one row of 16 positions.  The tap shift dy picks the patch row; the shift dx moves the 8-position window
// by one element, which a 16-byte LDS read cannot do.  Round 5: the patch row is stored TWICE — copy A = patch columns
// 0..15, copy B = patch columns 2..17 — so that the windows dx = -1 (A) and dx = +1 (B) are both aligned 16-byte reads
// into even-aligned register quads (an MFMA operand must start on an even register: with one copy + a fifth dword the
// dx = +1 window cost four moves per part and group on top of the read) and dx = 0 is four v_alignbit_b32 / v_perm_b32 of
// the two; no read has a bank conflict (the 4-byte fifth-dword reads were 4-way conflicted: the row pitch has to be a
// multiple of 4 dwords, so 32 rows hit 8 banks — 60 % of the round-4 kernel's LDS cycles).
// LDS rows are PERMUTED: channel 4q + e of the tile lives in row 16 e + q, so that the 16 staging lanes of a column
// group (q = 0..15, one float4 = channels 4q..4q+3 each) write 16 consecutive rows (row pitch 100 / 36 dwords = 36 mod 64:
// conflict-free 8-byte writes) and the 32 lanes of an MFMA operand read 32 consecutive rows (conflict-free);
// MFMA row / column l of wave w therefore stands for channel 4 (l & 15) + 2 w + (l >> 4) of the tile.
#include <type_traits>
#include <utility>
#include "common.h"
#include "wgrad_plan.h"                          // QH x QW position tile (4 rows: 108 MFMAs per wave per tile), CT

namespace hfagp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Both kernels: x [B][H][W][Cin] is the SHIFTED operand (staged with a halo, its channels are the MFMA rows), g the plain one (its
// channels are the MFMA columns).  tiles_h x tiles_w position tiles per sample (wgrad_plan.h: QH x QW positions).
struct Wg16Params {
    const float* x; const float* g; const float* styles;       // g [B][gH][gW][Cout]; styles [B][Cin] or null
    float* slabs;                       // [ksplit][Cout][Cin][9]: the parameter layout (tap = 3 (dy) + dx)
    // gH x gW = H x W = the position grid.  g's extents stay parameters of their own: read from H and W, the same kernel allocates
    // 210 vector registers instead of 204 (no spill, the same schedule otherwise)
    int B, H, W, gH, gW, Cin, Cout, tiles_h, tiles_w, ksplit;
};

constexpr int XR = QH + 2;                       // x patch: 6 rows of 18 columns (halo 1 + 16 + 1)
constexpr int XROW = 32;                         // bytes per patch row of one copy (16 columns)
constexpr int XCOPY = XR * XROW;                 // 192: copy A at 0, copy B at XCOPY
constexpr int XPITCH = 2 * XCOPY + 16;           // bytes per ci row of one part (400: 100 dwords = 36 mod 64, conflict-free b128);
                                                 // the 16 pad bytes absorb the writes of unit columns a copy does not hold
constexpr int GPITCH = QH * QW * 2 + 16;         // bytes per co row of one part (144: 36 dwords)
constexpr int XPART = CT * XPITCH, GPART = CT * GPITCH;
constexpr int BUF = 2 * XPART + 2 * GPART;       // one stage: x hi, x lo, g hi, g lo  (69 632 B; two stages)

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// four floats (consecutive positions of one channel) -> hi and lo part, two dwords each
__device__ __forceinline__ void split_run(float a, float b, float c, float d, uint2& hi, uint2& lo) {
    hi = make_uint2(pk_bf16(a, b), pk_bf16(c, d));
    lo = make_uint2(pk_bf16(a - __builtin_bit_cast(float, hi.x << 16), b - __builtin_bit_cast(float, hi.x & 0xffff0000u)),
                    pk_bf16(c - __builtin_bit_cast(float, hi.y << 16), d - __builtin_bit_cast(float, hi.y & 0xffff0000u)));
}

constexpr int popc3(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1); }
constexpr int rank3(int m, int i) { return popc3(m & ((1 << i) - 1)); }      // index of set bit i among the set bits
constexpr int nth3(int m, int j) {                                          // position of the j-th set bit
    int seen = 0;
    for (int i = 0; i < 3; ++i) if ((m >> i) & 1) { if (seen == j) return i; ++seen; }
    return 0;
}

// Epilogue of both kernels (round 5): the block's nine 64 x 64 accumulator tiles leave in the PARAMETER layout
// slab[co][ci][tap] — through LDS (the staging buffers are free by then): lane (co, rows ci) writes [co][ci * 9 + tap] with a
// row pitch of 64 * 9 + 1 floats (consecutive co -> consecutive banks), the block reads each co row back as 576 consecutive
// floats and stores them as one contiguous run.  The split-K reducer is then a plain sum of identical layouts (the slabs used to
// be [tap][ci][co] and the reducer a transposing gather: 28 us for 38-47 MB, launch after launch).
constexpr int EPI_PITCH = CT * 9 + 1;
constexpr int EPI_BYTES = CT * EPI_PITCH * 4;            // 147 712
__device__ __forceinline__ void store_slab_final(const f32x16 (&acc)[9], char* lds, float* slab, int Cin, int ci0, int co0,
                                                 int wi, int wj, int h, int l31, int tid) {
    const int run = min(CT, Cin - ci0) * 9;                  // floats per co row (a partial ci tile: Cin = 32 of the first SR layer)
    float* t32 = reinterpret_cast<float*>(lds);
    __syncthreads();                                         // every wave is done with the staging buffers
    const int cb = 4 * (l31 & 15) + 2 * wj + (l31 >> 4);     // MFMA column -> co of the tile (row permutation of the staging)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int ca = 4 * (rr & 15) + 2 * wi + (rr >> 4);               // MFMA row -> ci of the tile
            t32[cb * EPI_PITCH + ca * 9 + t] = acc[t][r];
        }
    __syncthreads();
    for (int c = 0; c < CT; ++c) {
        float* dst = slab + ((size_t)(co0 + c) * Cin + ci0) * 9;
        const float* src = t32 + c * EPI_PITCH;
        if (tid < run) dst[tid] = src[tid];
        if (tid + 256 < run) dst[tid + 256] = src[tid + 256];
        if (tid + 512 < run) dst[tid + 512] = src[tid + 512];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The pieces the two kernels below share.  Every one is inlined; where the compiled code dictates a form, the piece says so.

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in that order
template <class F, int... I>
__device__ __forceinline__ void static_for_seq(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_seq(f, std::make_integer_sequence<int, N>{}); }

// ---- staging.  A unit = one row x one column group (4 neighbouring positions) x one channel group (4 channels): 4 float4 loads,
// one per column.  x: 6 rows x 5 column groups (20 >= 18 columns) x 16 channel groups = 480 units, thread t owns units t and
// 256 + t (t < 224; the others repeat the last unit: same data, same addresses); g: 4 rows x 4 column groups x 16 channel groups =
// 256 units, one per thread.
struct Unit { int q, cg, row; };
constexpr int XUNITS = XR * 5 * 16;
__device__ __forceinline__ Unit x_unit(int u) { return {u & 15, (u >> 4) % 5, (u >> 4) / 5}; }
__device__ __forceinline__ Unit g_unit(int u) { return {u & 15, (u >> 4) & 3, u >> 6}; }
// (x_unit's two indices are computed by the caller before either is taken apart, and a unit's byte offset inside its image,
// ((row W + 4 cg) C + 4 q) 4, is written out in the kernels: as a function here it is simplified on its own before it is inlined, and
// both kernels come out with other address arithmetic.)
// LDS byte offsets of a unit's writes inside an x stage / a g stage, channel e = 0, hi part (+ 16 e XPITCH, + XPART: immediates).
// x unit (row, cg) holds patch columns 4cg .. 4cg+3.  Copy A keeps columns 0..15: an 8-byte write for cg <= 3; copy B
// keeps columns 2..17 at index col - 2: the pair's first dword goes to dword 2cg - 1 (cg >= 1), its second to dword
// 2cg (cg <= 3).  What a copy does not hold is written into the row's 16 pad bytes instead (no branch in a piece).
struct XOffsets { int oa, ob0, ob1; };
// (Filled in through a reference, and g_offset's sum in this order: returned by value / with the terms the other way round the
// kernels' prologues come out in another instruction order.)
__device__ __forceinline__ void x_offsets(const Unit& u, XOffsets& o) {
    const int base = u.q * XPITCH;
    o.oa = base + (u.cg <= 3 ? u.row * XROW + 8 * u.cg : 2 * XCOPY);
    o.ob0 = base + (u.cg >= 1 ? XCOPY + u.row * XROW + 4 * (2 * u.cg - 1) : 2 * XCOPY + 8);
    o.ob1 = base + (u.cg <= 3 ? XCOPY + u.row * XROW + 8 * u.cg : 2 * XCOPY + 12);
}
__device__ __forceinline__ int g_offset(const Unit& u) { return (u.row * QW + 4 * u.cg) * 2 + u.q * GPITCH; }

// ---- loads.  Raw buffer loads: the image of sample b is a buffer resource (4 scalar registers), a position is a 32-bit byte
// offset = (scalar tile origin) + (per-thread constant), and what is not there (outside the image, a null tile) gets the offset OOB
// past the end of any resource, for which the hardware returns zeros.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr unsigned OOB = 0xfffffff0u;
__device__ __forceinline__ rsrc_t image_rsrc(const float* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 load_b128(rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
// the four columns col0 .. col0 + 3 of a unit (C channels per position; base_t: the tile's scalar offset, uoff: the unit's own).
// `rowok` arrives as a value: with the row test written out in front of `&&` at the load, hipcc kept the short circuit of the up
// kernel's g loads as branches inside the tile loop, and a `vmcnt(0)` behind each (profiles/wgrad_lift/README.md).
__device__ __forceinline__ void load_unit(float4 (&r)[4], rsrc_t img, bool rowok, int col0, int W, int base_t, int C, int uoff) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool ok = rowok && (unsigned)(col0 + c) < (unsigned)W;
        r[c] = load_b128(img, ok ? (unsigned)(base_t + c * C * 4 + uoff) : OOB);
    }
}
// Styles [B][Cin] or none.  No styles: the resource is empty, the load returns zeros and `one` = 1 is added — a select on a
// uniform condition became a branch around the load, which costs hipcc its exact count of the loads in flight.
struct StyleSrc { rsrc_t rs; float one; };
__device__ __forceinline__ StyleSrc style_src(const float* styles, const float* any, int n) {
    return {image_rsrc(styles ? styles : any, styles ? (unsigned)n * 4u : 0u), styles ? 0.f : 1.f};
}
__device__ __forceinline__ float4 load_style(const StyleSrc& s, int chan0) {
    const float4 v = load_b128(s.rs, (unsigned)(chan0 * 4));
    return make_float4(v.x + s.one, v.y + s.one, v.z + s.one, v.w + s.one);
}
struct TileOrigin { int b, m0, n0; };
__device__ __forceinline__ TileOrigin tile_origin(int u, int tiles_w, int tiles_h) {
    const int tw = u % tiles_w, th = (u / tiles_w) % tiles_h;
    return {u / (tiles_w * tiles_h), th * QH, tw * QW};
}

// ---- conversion pieces: channel e of a unit (four float4, one per column) -> one split_run + its LDS writes.  x (times its
// style): an 8-byte write to copy A and two 4-byte writes to copy B, per part; g: an 8-byte write per part.
template <int e> __device__ __forceinline__ float chan(const float4& v) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
template <int e, int STAGE>                                  // STAGE: bytes between two x stages
__device__ __forceinline__ void commit_x_piece(char* lds, int stage, const XOffsets& o, const float4 (&r)[4], float sv) {
    uint2 hi, lo;
    split_run(chan<e>(r[0]) * sv, chan<e>(r[1]) * sv, chan<e>(r[2]) * sv, chan<e>(r[3]) * sv, hi, lo);
    char* row = lds + stage * STAGE + 16 * e * XPITCH;       // (the stage's address after the split, as both kernels had it)
    *reinterpret_cast<uint2*>(row + o.oa) = hi;
    *reinterpret_cast<uint2*>(row + o.oa + XPART) = lo;
    *reinterpret_cast<unsigned*>(row + o.ob0) = hi.x;
    *reinterpret_cast<unsigned*>(row + o.ob1) = hi.y;
    *reinterpret_cast<unsigned*>(row + o.ob0 + XPART) = lo.x;
    *reinterpret_cast<unsigned*>(row + o.ob1 + XPART) = lo.y;
}
template <int e>
__device__ __forceinline__ void commit_g_piece(char* gunit, const float4 (&r)[4]) {       // gunit: g stage + g_offset of the unit
    uint2 hi, lo;
    split_run(chan<e>(r[0]), chan<e>(r[1]), chan<e>(r[2]), chan<e>(r[3]), hi, lo);
    char* dst = gunit + 16 * e * GPITCH;
    *reinterpret_cast<uint2*>(dst) = hi;
    *reinterpret_cast<uint2*>(dst + GPART) = lo;
}

// per-lane fragment base (bytes inside a stage): LDS row 32 w + l31 of the wave's tile, columns 8h..
__device__ __forceinline__ int frag_base(int w, int l31, int h, int pitch) { return (32 * w + l31) * pitch + 8 * h * 2; }
// fragments of one group as they come out of LDS: copy A / copy B window of the patch row, hi and lo part
struct Raw { u32x4 ha, hb, la, lb; };
__device__ __forceinline__ Raw read_a(const char* xst, int abase, int prow) {
    const char* ar = xst + abase + prow * XROW;
    Raw r;
    r.ha = *reinterpret_cast<const u32x4*>(ar);
    r.hb = *reinterpret_cast<const u32x4*>(ar + XCOPY);
    r.la = *reinterpret_cast<const u32x4*>(ar + XPART);
    r.lb = *reinterpret_cast<const u32x4*>(ar + XPART + XCOPY);
    return r;
}

// ---- the K loop.  A GROUP = one patch row of one K step (tile row kr, patch row kr + dy): 4 LDS reads, the dx windows, the MFMAs
// of the taps that row serves.  Which rows and windows a kernel (or a phase of it) uses, and which accumulator a tap lands in:
//   dym / dxm: bit i set = patch-row / window offset i is used (shift i - 1);  slot(dy, dx): accumulator of that tap.
template <int DYM, int DXM>
struct Taps3x3 {                                             // 7, 7: the nine taps in (dy, dx) order
    static constexpr int dym = DYM, dxm = DXM;
    static constexpr int slot(int dy, int dx) { return rank3(DYM, dy) * popc3(DXM) + rank3(DXM, dx); }
};
template <int PP, int PQ>
struct TapsUp {                                              // parity image (PP, PQ) of the up-conv: shifts -1 / 0, or 0 alone
    static constexpr int dym = PP ? 2 : 3, dxm = PQ ? 2 : 3;
    // (dy = 1: shift 0 -> sy = 0; dy = 0: shift -1 -> sy = 1, the same for dx; tap slot = 3 ky + kx, ky = PP + 2 sy, kx = PQ + 2 sx)
    static constexpr int slot(int dy, int dx) { return 3 * (PP + 2 * (1 - dy)) + PQ + 2 * (1 - dx); }
};
// the fragments a group consumes: the x windows and the g row of its K step, hi and lo part
struct Group { Raw a; u32x4 bh, bl; };
template <class Taps>
__device__ __forceinline__ Group read_group0(const char* xst, int abase, const char* gfrag) {        // gfrag: g stage + its frag_base
    return {read_a(xst, abase, nth3(Taps::dym, 0)), *reinterpret_cast<const u32x4*>(gfrag), *reinterpret_cast<const u32x4*>(gfrag + GPART)};
}
// the MFMAs of one group
template <class Taps, int dy>
__device__ __forceinline__ void mfma_group(f32x16 (&acc)[9], const Raw& w, const u32x4& bh, const u32x4& bl) {
    constexpr int DXM = Taps::dxm;
    u32x4 ah[3], al[3];                           // the three dx windows (start column 8h + dx)
    ah[0] = w.ha; al[0] = w.la; ah[2] = w.hb; al[2] = w.lb;
    if constexpr ((DXM >> 1) & 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {             // columns 8h+1+2e, 8h+2+2e = high half of A's dword e, low half of B's
            ah[1][e] = __builtin_amdgcn_alignbit(w.hb[e], w.ha[e], 16);
            al[1][e] = __builtin_amdgcn_alignbit(w.lb[e], w.la[e], 16);
        }
    }
    // product-major (hi.hi, lo.hi, hi.lo): the three MFMAs of one accumulator are up to two other MFMAs apart
#pragma unroll
    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
            if ((DXM >> dx) & 1) {
                const int t = Taps::slot(dy, dx);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pr == 1 ? al[dx] : ah[dx]),
                                                                 __builtin_bit_cast(bf16x8, pr == 2 ? bl : bh), acc[t], 0, 0, 0);
            }
}
// Group G of a K loop with read-ahead: the LDS reads of group G + 1, the MFMAs of group G, then the pieces P = G, G + NG, ... < NP of
// the conversion that rides along (piece(integral_constant<int, P>)); a sched_barrier per group pins that order.
template <class Taps, int G, int NP, class Piece>
__device__ __forceinline__ void group_step(f32x16 (&acc)[9], Group& cur, const char* xst, int abase, const char* gfrag, Piece&& piece) {
    constexpr int DYM = Taps::dym, NDY = popc3(DYM), NG = QH * NDY;
    constexpr int kr = G / NDY, dy = nth3(DYM, G % NDY);
    constexpr int G1 = G + 1, kr1 = G1 / NDY, dy1 = nth3(DYM, G1 % NDY);
    Group nxt = cur;
    if constexpr (G1 < NG) {
        nxt.a = read_a(xst, abase, kr1 + dy1);
        if constexpr (kr1 != kr) {
            nxt.bh = *reinterpret_cast<const u32x4*>(gfrag + kr1 * QW * 2);
            nxt.bl = *reinterpret_cast<const u32x4*>(gfrag + GPART + kr1 * QW * 2);
        }
    }
    mfma_group<Taps, dy>(acc, cur.a, cur.bh, cur.bl);
    static_for<(NP > G ? (NP - G + NG - 1) / NG : 0)>([&](auto j) __attribute__((always_inline)) {
        piece(std::integral_constant<int, G + decltype(j)::value * NG>{});
    });
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
}

// The 3x3 kernel.  DYM / DXM: the masks of Taps3x3; the one instance is <7, 7> (nine taps).
//
// Schedule (round 5).  One wave per SIMD (144 accumulator registers), so nothing but this wave's own instruction stream can
// fill the matrix pipe's shadow.  PMC of the round-4 kernel (profiles/r05_pmc/wgrad_256_256_at256.txt): 5.4 vector-ALU
// instructions per MFMA, MFMA pipe 0.39 busy, 60 % of the LDS cycles bank conflicts.  That kernel ran the K loop of tile u
// (108 MFMAs), THEN converted + wrote tile u+1 (≈ 270 VALU + 24 LDS writes with the pipe idle), then a barrier.  Now
//   * the staging work of tile u+1 is cut into 12 pieces (unit x channel: one split_run + its LDS writes) and piece g is
//     issued inside group g of the K loop (a group = one patch row of one K step: 4 LDS reads, 8 v_perm, 9 MFMAs), the LDS
//     reads of group g+1 in front of the MFMAs of group g (a sched_barrier per group pins that);
//   * which needs tile u+1's loads to have LANDED when the K loop of tile u starts: the loads run a whole tile ahead of the
//     conversion (two register sets, the tile loop unrolled by two so that both are statically indexed);
//   * the loop body has NO branch: hipcc's s_waitcnt insertion counts outstanding loads exactly only along straight-line
//     code (with `if (u + 2 < u_end) fetch(...)` every conversion piece waited for vmcnt(0), i.e. for the loads just
//     issued).  A block therefore always runs an even number of phases; tiles past its range are NULL tiles — every load
//     out of range — and contribute zeros, and every phase converts "the next tile" whether or not there is one;
//   * raw buffer loads: a position is a 32-bit offset = scalar tile origin + per-thread constant, and an out-of-image (or
//     null-tile) position gets an offset past the end of the resource, for which the hardware returns zeros: no masks (12
//     registers and 48 multiplies per tile), no 64-bit address arithmetic, no memory traffic for what is not there.
template <int DYM, int DXM>
__global__ void __launch_bounds__(256, 1) wgrad_bf16_kernel(const Wg16Params p) {
    using Taps = Taps3x3<DYM, DXM>;
    constexpr int NG = QH * popc3(DYM);               // groups of the K loop
    static_assert(popc3(DYM) * popc3(DXM) == 9, "nine accumulators, and the final-layout epilogue is written for the nine-tap kernel");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;     // wave tile: ci rows 32*wi.., co cols 32*wj..
    const int h = lane >> 5, l31 = lane & 31;
    const int ci0 = blockIdx.x * CT, co0 = blockIdx.y * CT, ks = blockIdx.z;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int units = p.B * p.tiles_h * p.tiles_w;
    const int u_begin = (int)(((long long)units * ks) / p.ksplit), u_end = (int)(((long long)units * (ks + 1)) / p.ksplit);

    // ---- staging: two x units and one g unit per thread.  Nothing in fetch() consumes a loaded value, so the loads stay in flight
    // under the MFMAs.
    float4 rx[2][2][4], rg[2][4], sx[2][2];       // [register set][...]
    const int ux0 = tid, ux1 = min(tid + 256, XUNITS - 1);
    const Unit xu[2] = {x_unit(ux0), x_unit(ux1)}, gu = g_unit(tid);
    XOffsets xo[2];
    x_offsets(xu[0], xo[0]);
    x_offsets(xu[1], xo[1]);
    const int og = 2 * XPART + g_offset(gu);

    const int xoff[2] = {((xu[0].row * p.W + 4 * xu[0].cg) * p.Cin + 4 * xu[0].q) * 4, ((xu[1].row * p.W + 4 * xu[1].cg) * p.Cin + 4 * xu[1].q) * 4};
    const int goff = ((gu.row * p.gW + 4 * gu.cg) * p.Cout + 4 * gu.q) * 4;
    const unsigned abytes = (unsigned)(p.H * p.W * p.Cin) * 4u, bbytes = (unsigned)(p.gH * p.gW * p.Cout) * 4u;
    const StyleSrc styles = style_src(p.styles, p.x, p.B * p.Cin);
    auto fetch = [&](int u, auto set_tag) __attribute__((always_inline)) {
        constexpr int S = decltype(set_tag)::value;
        const bool live = u < u_end;                         // (a null tile: every offset out of range)
        const TileOrigin t = tile_origin(live ? u : u_end - 1, p.tiles_w, p.tiles_h);
        const rsrc_t ra = image_rsrc(p.x + (size_t)t.b * p.H * p.W * p.Cin + ci0, live ? abytes - 4u * ci0 : 0u);
        const rsrc_t rb = image_rsrc(p.g + (size_t)t.b * p.gH * p.gW * p.Cout + co0, live ? bbytes - 4u * co0 : 0u);
        const int abase_t = (((t.m0 - 1) * p.W + t.n0 - 1) * p.Cin) * 4, bbase_t = ((t.m0 * p.gW + t.n0) * p.Cout) * 4;      // scalar
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool rowok = (unsigned)(t.m0 - 1 + xu[k].row) < (unsigned)p.H;
            sx[S][k] = load_style(styles, t.b * p.Cin + ci0 + 4 * xu[k].q);
            load_unit(rx[S][k], ra, rowok, t.n0 - 1 + 4 * xu[k].cg, p.W, abase_t, p.Cin, xoff[k]);
        }
        load_unit(rg[S], rb, t.m0 + gu.row < p.gH, t.n0 + 4 * gu.cg, p.gW, bbase_t, p.Cout, goff);
    };
    // piece P of the conversion of register set S into LDS stage `buf`: P = 0..3 channel e of x unit 0, 4..7 of x unit 1,
    // 8..11 of the g unit
    auto commit_piece = [&](int buf, auto set_tag, auto piece_tag) __attribute__((always_inline)) {
        constexpr int S = decltype(set_tag)::value, P = decltype(piece_tag)::value, e = P & 3;
        char* base = lds + buf * BUF;
        if constexpr (P < 8) commit_x_piece<e, BUF>(lds, buf, xo[P >> 2], rx[S][P >> 2], chan<e>(sx[S][P >> 2]));
        else commit_g_piece<e>(base + og, rg[S]);
    };
    auto commit_all = [&](int buf, auto set_tag) __attribute__((always_inline)) {
        static_for<12>([&](auto piece_tag) __attribute__((always_inline)) { commit_piece(buf, set_tag, piece_tag); });
    };

    const int abase = frag_base(wi, l31, h, XPITCH), bbase = 2 * XPART + frag_base(wj, l31, h, GPITCH);

    // phase: tile u sits in stage S (converted from register set S, which is free again); register set 1 - S holds tile u + 1 and
    // is converted into the other stage inside the K loop (12 pieces over NG groups: piece P rides in group P % NG); groups in
    // (kr, dy) order
    auto phase = [&](int u, auto s_tag) __attribute__((always_inline)) {
        constexpr int S = decltype(s_tag)::value;
        fetch(u + 2, s_tag);
        const char* st = lds + S * BUF;
        Group cur = read_group0<Taps>(st, abase, st + bbase);
        auto piece = [&](auto piece_tag) __attribute__((always_inline)) { commit_piece(S ^ 1, std::integral_constant<int, 1 - S>{}, piece_tag); };
        static_for<NG>([&](auto g) __attribute__((always_inline)) { group_step<Taps, decltype(g)::value, 12>(acc, cur, st, abase, st + bbase, piece); });
        __syncthreads();
    };

    fetch(u_begin, std::integral_constant<int, 0>{});
    fetch(u_begin + 1, std::integral_constant<int, 1>{});
    commit_all(0, std::integral_constant<int, 0>{});
    __syncthreads();
    for (int u = u_begin; u < u_end; u += 2) {               // (an odd tile count ends with a null tile: zeros)
        phase(u, std::integral_constant<int, 0>{});
        phase(u + 1, std::integral_constant<int, 1>{});
    }
    // ---- slab [Cout][Cin][9] (the parameter layout): C/D layout row = (r&3) + 8*(r>>2) + 4*h (ci), col = lane&31 (co)
    store_slab_final(acc, lds, p.slabs + (size_t)ks * 9 * p.Cin * p.Cout, p.Cin, ci0, co0, wi, wj, h, l31, tid);
}

// ---------------------------------------------------------------------------------------------------------------
// Weight gradient of the UP-SAMPLING conv in one kernel (round 5; before: four launches of the kernel above, one per parity image
// of the y_t gradient, each staging the x tile again — 1.3 ms of the generator-tuned step at 0.11-0.16 of the MFMA ceiling).
//   dW[ky][kx][ci][co] = sum_{b,i,j} (x s)[b][i][j][ci] * g_t[b][2i + ky][2j + kx][co]
//                      = sum_{b,m,n} (x s)[b][m - sy][n - sx][ci] * g_par[p][q][b][m][n][co],   ky = p + 2 sy, kx = q + 2 sx
// on the (H+1) x (W+1) grid of a parity image: the SHIFTED operand is x (shifts -1 / 0: halo on top and on the left, staged
// ONCE per position tile), the plain operand is the tile of ONE parity image, and a tile is four PHASES — parity (1,1): 1 tap,
// (0,1) and (1,0): 2 taps, (0,0): 4 taps — that share the nine accumulators of the 3x3 kernel (tap slot = 3 ky + kx).
// Same pipeline as above, per phase instead of per tile: the gradient tile of (tile u+1, phase f) is loaded at the start of (tile u,
// phase f) (four register sets: a whole tile of latency) and converted inside the K loop of the phase before its own (4 pieces); the
// x patch of tile u+1 is loaded at the start of tile u and converted inside its last, 4-tap phase (8 pieces).  The loop body (one tile = four
// phases) has no branch; phases past the block's range load zeros.
struct WgUpParams {
    const float* x; const float* g; const float* styles;      // g = [2][2][B][H+1][W+1][Cout]
    float* slabs;                                             // [ksplit][Cout][Cin][9]
    int B, H, W, Cin, Cout, tiles_h, tiles_w, ksplit;
};
constexpr int UBX = 2 * XPART, UBG = 2 * GPART;               // one x stage (hi, lo), one g stage
constexpr int up_parity(int J) { return J == 0 ? 3 : J == 1 ? 1 : J == 2 ? 2 : 0; }      // phase J of a tile -> parity image 2 p + q

__global__ void __launch_bounds__(256, 1) wgrad_up_bf16_kernel(const WgUpParams p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];     // [x stage 0][x stage 1][g stage 0][g stage 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int h = lane >> 5, l31 = lane & 31;
    const int ci0 = blockIdx.x * CT, co0 = blockIdx.y * CT, ks = blockIdx.z;
    const int gH = p.H + 1, gW = p.W + 1;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int units = p.B * p.tiles_h * p.tiles_w;
    const int u_begin = (int)(((long long)units * ks) / p.ksplit), u_end = (int)(((long long)units * (ks + 1)) / p.ksplit);

    float4 rx[2][4], sx[2], rg[4][4];                          // x: one register set (two units); g: [set = phase of the tile][column]
    const int ux0 = tid, ux1 = min(tid + 256, XUNITS - 1);
    const Unit xu[2] = {x_unit(ux0), x_unit(ux1)}, gu = g_unit(tid);
    XOffsets xo[2];
    x_offsets(xu[0], xo[0]);
    x_offsets(xu[1], xo[1]);
    const int og = g_offset(gu);

    const int xoff[2] = {((xu[0].row * p.W + 4 * xu[0].cg) * p.Cin + 4 * xu[0].q) * 4, ((xu[1].row * p.W + 4 * xu[1].cg) * p.Cin + 4 * xu[1].q) * 4};
    const int goff = ((gu.row * gW + 4 * gu.cg) * p.Cout + 4 * gu.q) * 4;
    const unsigned xbytes = (unsigned)(p.H * p.W * p.Cin) * 4u, gbytes = (unsigned)(gH * gW * p.Cout) * 4u;
    const StyleSrc styles = style_src(p.styles, p.x, p.B * p.Cin);
    const size_t par_stride = (size_t)p.B * gH * gW * p.Cout;        // floats between parity images

    // x patch of tile u: rows m0-1 .. m0+4, columns n0-1 .. n0+18 (5 column groups of 4)
    auto fetch_x = [&](int u) __attribute__((always_inline)) {
        const bool live = u < u_end;
        const TileOrigin t = tile_origin(live ? u : u_end - 1, p.tiles_w, p.tiles_h);
        const rsrc_t ra = image_rsrc(p.x + (size_t)t.b * p.H * p.W * p.Cin + ci0, live ? xbytes - 4u * ci0 : 0u);
        const int base_t = (((t.m0 - 1) * p.W + t.n0 - 1) * p.Cin) * 4;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            // (shifts -1 / 0: five patch rows; a partial ci tile — Cin = 32 — loads zeros for the channels it does not have)
            const bool rowok = (unsigned)(t.m0 - 1 + xu[k].row) < (unsigned)p.H && xu[k].row < XR - 1 && ci0 + 4 * xu[k].q < p.Cin;
            sx[k] = load_style(styles, t.b * p.Cin + ci0 + 4 * xu[k].q);
            load_unit(rx[k], ra, rowok, t.n0 - 1 + 4 * xu[k].cg, p.W, base_t, p.Cin, xoff[k]);
        }
    };
    // gradient tile of (tile u, phase J) into register set J
    auto fetch_g = [&](int u, auto j_tag) __attribute__((always_inline)) {
        constexpr int PAR = up_parity(decltype(j_tag)::value), S = decltype(j_tag)::value;
        const bool live = u < u_end;
        const TileOrigin t = tile_origin(live ? u : u_end - 1, p.tiles_w, p.tiles_h);
        const rsrc_t rb = image_rsrc(p.g + PAR * par_stride + (size_t)t.b * gH * gW * p.Cout + co0, live ? gbytes - 4u * co0 : 0u);
        load_unit(rg[S], rb, t.m0 + gu.row < gH, t.n0 + 4 * gu.cg, gW, ((t.m0 * gW + t.n0) * p.Cout) * 4, p.Cout, goff);
    };
    // conversion pieces: x piece P = 0..7 (unit P >> 2, channel P & 3) into x stage `xs`; g piece e of set S into g stage `gs`
    auto x_piece = [&](int xs, auto piece_tag) __attribute__((always_inline)) {
        constexpr int P = decltype(piece_tag)::value;
        commit_x_piece<(P & 3), UBX>(lds, xs, xo[P >> 2], rx[P >> 2], chan<(P & 3)>(sx[P >> 2]));
    };
    auto g_piece = [&](int gs, auto set_tag, auto e_tag) __attribute__((always_inline)) {
        commit_g_piece<decltype(e_tag)::value>(lds + 2 * UBX + gs * UBG + og, rg[decltype(set_tag)::value]);
    };

    const int abase = frag_base(wi, l31, h, XPITCH), bbase = frag_base(wj, l31, h, GPITCH);

    // one phase: K loop of (x stage xs, g stage J & 1) for the parity image of phase J; riding along: the four g pieces of the NEXT
    // phase (register set (J + 1) & 3 -> g stage (J + 1) & 1) and, in the last phase of a tile, the eight x pieces of the next tile
    auto phase = [&](int xs, auto j_tag) __attribute__((always_inline)) {
        constexpr int J = decltype(j_tag)::value;                      // phase of the tile: parities in the order 3, 1, 2, 0
        using Taps = TapsUp<(up_parity(J) >> 1), (up_parity(J) & 1)>;
        constexpr int NG = QH * popc3(Taps::dym);
        constexpr int NP = J == 3 ? 12 : 4;                            // pieces that ride in this phase (the 4-tap phase also converts x)
        const char* xst = lds + xs * UBX;
        const char* gst = lds + 2 * UBX + (J & 1) * UBG;
        Group cur = read_group0<Taps>(xst, abase, gst + bbase);
        auto piece = [&](auto k_tag) __attribute__((always_inline)) {
            constexpr int K = decltype(k_tag)::value;
            if constexpr (K < 4) g_piece((J + 1) & 1, std::integral_constant<int, (J + 1) & 3>{}, k_tag);
            else x_piece(xs ^ 1, std::integral_constant<int, K - 4>{});
        };
        static_for<NG>([&](auto g) __attribute__((always_inline)) { group_step<Taps, decltype(g)::value, NP>(acc, cur, xst, abase, gst + bbase, piece); });
        __syncthreads();
    };

    // prologue: x of the first tile and the gradient tiles of its four phases (register set = phase); first x patch and first g tile
    // converted.  In the loop the gradient tile of (tile u+1, phase J) is loaded at the start of (tile u, phase J) — a whole tile
    // ahead: with two sets / two phases ahead (first version) a phase of 12 - 24 MFMAs was over before its successor's loads had
    // landed, SQ_WAIT_ANY 43 % of the wave cycles, MFMA pipe 0.27 busy — and converted inside the phase before its own.
    fetch_x(u_begin);
    static_for<4>([&](auto j_tag) __attribute__((always_inline)) { fetch_g(u_begin, j_tag); });
    static_for<8>([&](auto piece_tag) __attribute__((always_inline)) { x_piece(0, piece_tag); });
    static_for<4>([&](auto e_tag) __attribute__((always_inline)) { g_piece(0, std::integral_constant<int, 0>{}, e_tag); });
    __syncthreads();
    int xs = 0;
    for (int u = u_begin; u < u_end; ++u) {
        // (set J held tile u's phase-J tile, converted during phase J - 1: free when phase J starts)
        fetch_x(u + 1);                                                                          // converted inside phase 3
        static_for<4>([&](auto j_tag) __attribute__((always_inline)) {
            fetch_g(u + 1, j_tag);
            phase(xs, j_tag);
        });
        xs ^= 1;
    }
    store_slab_final(acc, lds, p.slabs + (size_t)ks * 9 * p.Cin * p.Cout, p.Cin, ci0, co0, wi, wj, h, l31, tid);
}

// host side: all nine taps of the up-sampling conv in one launch; slabs [ksplit][Cout][Cin][9], tap = 3 ky + kx
int launch_wgrad_up_bf16(const HfagpWgradArgs* a, hipStream_t s) {
    WgUpParams p{};
    p.x = a->x; p.g = a->g; p.styles = a->styles; p.slabs = a->workspace;
    p.B = a->B; p.H = a->H; p.W = a->W; p.Cin = a->Cin; p.Cout = a->Cout; p.ksplit = a->ksplit;
    p.tiles_h = (a->H + 1 + QH - 1) / QH; p.tiles_w = (a->W + 1 + QW - 1) / QW;
    const size_t lds = (2 * UBX + 2 * UBG) > EPI_BYTES ? (size_t)(2 * UBX + 2 * UBG) : (size_t)EPI_BYTES;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_up_bf16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    wgrad_up_bf16_kernel<<<dim3((a->Cin + CT - 1) / CT, a->Cout / CT, a->ksplit), 256, lds, s>>>(p);
    return check_launch("conv_wgrad (up-sampling conv, split bf16)");
}

template <int DYM, int DXM>
static int launch_wg16(const Wg16Params& p, dim3 grid, hipStream_t s) {
    const size_t lds = 2 * BUF > EPI_BYTES ? (size_t)(2 * BUF) : (size_t)EPI_BYTES;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_bf16_kernel<DYM, DXM>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    wgrad_bf16_kernel<DYM, DXM><<<grid, 256, lds, s>>>(p);
    return check_launch("conv_wgrad (split bf16)");
}

// host side (called by hfagp_conv_wgrad where wgrad_split16 holds, wgrad_plan.h): the 3x3 conv
int launch_wgrad3x3_bf16(const HfagpWgradArgs* a, hipStream_t s) {
    Wg16Params p{};
    p.x = a->x; p.g = a->g; p.styles = a->styles; p.slabs = a->workspace;
    p.B = a->B; p.H = a->H; p.W = a->W; p.gH = a->H; p.gW = a->W; p.Cin = a->Cin; p.Cout = a->Cout; p.ksplit = a->ksplit;
    p.tiles_h = (a->H + QH - 1) / QH; p.tiles_w = (a->W + QW - 1) / QW;
    return launch_wg16<7, 7>(p, dim3(a->Cin / CT, a->Cout / CT, a->ksplit), s);
}

}  // namespace hfagp
