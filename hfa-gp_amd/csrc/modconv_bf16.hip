// Modulated convolution on the 16-bit matrix pipe (v_mfma_f32_32x32x16_{f16,bf16}, gfx950) with SPLIT operands:
// every fp32 operand is the sum of 16-bit parts, each the round-to-nearest value of the residual left by the parts
// before it, and a product is the sum of the part products above the target weight, accumulated in fp32.  Operand
// kinds (template parameter KD):
//   KD = 4  F16X3 (default)  fp16 hi + lo (11 + 11 mantissa bits), hi.hi + lo.hi + hi.lo:      ~2^-22 per product
//   KD = 2  BF16X3           bf16 hi + lo ( 8 +  8 bits),          the same three products:      ~2^-16
//   KD = 3  BF16X6           bf16 hi + mid + lo,                   six products:                 ~2^-23
//   KD = 1  F16              one fp16 rounding,                    ONE product (EG3D's fp16 blocks): ~2^-11
// The 16-bit pipe is 16x the fp32 one, so the 3-product kinds have 5.3x the MFMA ceiling of the exact kernel
// (modconv.hip).  The fp16 kinds carry a range guard (style_range_guard) and a saturating split.
//
//   same implicit GEMM as modconv.hip: M = 8x16 output positions, N = 128 output channels, K = taps x Cin in
//   chunks of 16 channels (= one MFMA K step).  The activations are read as fp32, scaled by the style, split and
//   written to LDS as part images [part][position][16 ch + 16 B pad] (48-B pitch, row pitch 32 positions: every
//   16-lane group of a ds_read_b128 covers 16 distinct 16-B slots).
//   The weights are pre-split (hfagp_weight_prep_prec) into [part][tap][Cin/8][Cout][8], which is the B-operand
//   fragment order: a lane's 8 K values are one 16-B load, straight from L2 into the fragment registers through a
//   ring that stays 3 (F16: 6) taps ahead of the MFMAs.  The patch of the next chunk is converted under the last
//   taps of the current one into the other LDS buffer: one barrier per chunk.
#include <atomic>
#include <type_traits>
#include "conv16_common.h"

namespace hfagp {

// IO: fp16 STORAGE of the activations (hfagp.h x_f16 / y_f16; KD = 1 only): bit 0 = x is fp16 (staging copies the halves
// and applies the style with packed fp16 multiplies), bit 1 = y is written as fp16
template <int KD, int TM, int NTAPS, int IO = 0>
__global__ void __launch_bounds__(256, 2) modconv_bf16_kernel(const ConvParams p, const int phase0) {
    constexpr int NP = kind_parts_a(KD), NPB = kind_parts(KD);    // parts of the activations (LDS patch) / of the weight image
    constexpr bool F16 = kind_f16(KD);
    constexpr bool XH = (IO & 1) != 0, YH = (IO & 2) != 0;
    constexpr int XB = XH ? 2 : 4;                       // bytes per input element
    static_assert((IO & 3) == 0 || KD == 1, "fp16 storage goes with the single-pass fp16 arithmetic");
    // IO bit 2: the epilogue this kernel had before its loads were batched (developer switch HFAGP_DEV_CONV_EPILOGUE_LEGACY=1,
    // instantiated for the F16X3 forward 3x3 conv only: launch_modconv_bf16)
    constexpr bool ELEG = (IO & 4) != 0;
    static_assert(!ELEG || (KD == 4 && NTAPS == 9 && IO == 4), "the legacy epilogue is kept for one instantiation");
    // wave grid WM x WN over the 128 x 128 block tile; TM here is the M tiles per wave for WN = 2
    constexpr int WN = 2, WM = 4 / WN, TN = 4 / WN, TMW = 4 / WM, BM = 128, PH = BM / PW;
    static_assert(TM == 2, "block tile is 128 positions");
    constexpr int LPWB = RowPitch<NP>::value;
    constexpr int APOS = (PH + 2) * LPWB;                 // positions of the staged patch
    constexpr int A_PART = APOS * APITCH, A_BUF = NP * A_PART;
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    char* As = lds_raw;                                   // [2][NP][APOS][48 B]
    float* Ss = reinterpret_cast<float*>(lds_raw + 2 * A_BUF);   // [Cin] styles of this sample (or ones)

    // NTAPS = 0: the adjoint of the up-sampling conv (mode CONVS2_BWD) MERGED — the four parity phases (4 | 2 | 2 | 1 taps, each
    // reading its own parity image of the y_t gradient) run one after the other in this block into ONE accumulator set, so the
    // result is written once (round 3 launched the three tap counts separately, each into its own slab, and summed the slabs
    // in splitk_epilogue_kernel: 4 launches and 4 x the output traffic per layer).  All four phases share the output grid.
    constexpr bool MERGED_S2 = NTAPS == 0;
    const Phase& ph = p.phase[MERGED_S2 ? 0 : phase0 + blockIdx.y];   // every phase of one launch has NTAPS taps
    // (readfirstlane: the divisions by run-time values are done on the vector ALU; without it every index derived
    // from the block coordinates stays in VGPRs and the uniform address arithmetic of the K loop — chunk x Cout
    // products, clamps — is issued as quarter-rate vector multiplies between the MFMAs)
    unsigned id = p.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tn_blk = __builtin_amdgcn_readfirstlane(id % p.tiles_n); id /= p.tiles_n;
    const int tw = __builtin_amdgcn_readfirstlane(id % p.tiles_w);     id /= p.tiles_w;
    const int th = __builtin_amdgcn_readfirstlane(id % p.tiles_h);     id /= p.tiles_h;
    const int b = __builtin_amdgcn_readfirstlane(id % p.B);            id /= p.B;
    const int ks = __builtin_amdgcn_readfirstlane(id);
    const int m0 = th * PH, n0 = tw * PW, co0 = tn_blk * BNB;
    if (m0 >= ph.mh || n0 >= ph.mw) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int h = lane >> 5, l31 = lane & 31;

    const int c_begin = __builtin_amdgcn_readfirstlane((int)(((long long)p.nchunks * ks) / p.ksplit));
    const int c_end = __builtin_amdgcn_readfirstlane((int)(((long long)p.nchunks * (ks + 1)) / p.ksplit));

    // ---- A staging: float4 (4 channels of one position) per slot, 4 slots per position.  Everything is
    // branch-free: a slot outside the image (zero padding) reads element 0 and is multiplied by 0, a thread past
    // the end of the patch repeats the last slot (same value to the same LDS address), and addresses are a
    // uniform base + a 32-bit per-lane byte offset (global_load with an SGPR base: no 64-bit VALU address math).
    const int npatch = p.ph * p.pw;
    constexpr int A_PER_T = ((PH + 2) * (PW + 2) * 4 + 255) / 256;
    static_assert(A_PER_T == 3, "the staging schedule below is written for three slots per thread");
    float4 ra[A_PER_T];
    const char* xb = reinterpret_cast<const char*>(p.x) + (ph.in_off + (long long)b * p.x_batch_stride) * XB;   // (MERGED_S2: per phase)
    for (int i = tid; i < p.Cin; i += 256) Ss[i] = p.styles ? p.styles[(size_t)b * p.Cin + i] : 1.f;
    float sback = 1.f, sdown = 1.f;                      // 2^e, 2^-e of the fp16 range guard (1 for the bf16 kinds)
    if constexpr (F16) sdown = style_range_guard(p.styles ? p.styles + (size_t)b * p.Cin : nullptr, p.Cin, lane, &sback, p.x_absmax, p.w_absmax);
    unsigned aoff[A_PER_T];
    int lds_a[A_PER_T], soff[A_PER_T];
    float amask[A_PER_T];
#pragma unroll
    for (int k = 0; k < A_PER_T; ++k) {
        const int idx = min(tid + k * 256, npatch * 4 - 1);
        const int pix = idx >> 2, q = idx & 3;
        lds_a[k] = ((pix / p.pw) * LPWB + pix % p.pw) * APITCH + 8 * q;
        const int iy = m0 + p.dymin + pix / p.pw, ix = n0 + p.dxmin + pix % p.pw;
        const bool inside = iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w;
        aoff[k] = inside ? (unsigned)((iy * p.in_w + ix) * p.Cin + 4 * q) * (unsigned)XB : 0u;   // bytes, < 2^32 per image
        amask[k] = inside ? sdown : 0.f;          // zero padding and the fp16 range guard in one factor
        soff[k] = 4 * q;
    }
    auto load_a = [&](int chunk) __attribute__((always_inline)) { a16_load<XH>(ra, xb, chunk, aoff); };
    // slot K of the staged patch of `chunk`: scale by the style, split, write the parts to LDS buffer BUF
    auto store_a = [&](int chunk, auto buf_tag, auto k_tag) __attribute__((always_inline)) {
        constexpr int BUF = decltype(buf_tag)::value, k = decltype(k_tag)::value;
        a16_store<KD, XH>(As + BUF * A_BUF, A_PART, lds_a[k], amask[k], *reinterpret_cast<const float4*>(Ss + chunk * CKB + soff[k]), ra[k]);
    };

    // ---- B operand: straight from global/L2 into the fragment registers (no LDS, no barrier): a lane's fragment
    // is 16 contiguous bytes of the split image and lanes 0-31 / 32-63 of a fragment read two contiguous 512-B
    // runs, so the loads are full 128-B lines.  A ring of RB (2..4) fragment sets keeps the loads RB items ahead of the
    // MFMAs that consume them (item = one tap of one K chunk).
    const char* wb = reinterpret_cast<const char*>(p.wt);
    const int cq8 = p.Cin >> 3;
    // Cout = 96 (toRGB) runs on the same 128-wide tile: the lanes of its last 32 columns read the first 32 entries of
    // the NEXT image row (the caller pads the buffer by 512 B for the very last row), their accumulators are never
    // stored.  (A separate padded pitch for the image cost 66 VGPRs in the 9-tap kernel: spills.)
    const int part_stride = p.wtaps * cq8 * p.Cout;                           // uint4 per part
    unsigned bth[TN];                                                         // per-lane byte offset of a fragment
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) bth[tn] = (unsigned)(h * p.Cout + co0 + (wn * TN + tn) * 32 + l31) * 16u;
    int wtap[MAXTAPS];                                                        // tap table -> registers, once
#pragma unroll
    for (int t = 0; t < MAXTAPS; ++t) wtap[t] = t < ph.ntaps ? ph.widx[t] * cq8 * p.Cout : 0;

    // ---- per-lane fragment address of each M tile (bytes inside one part image, tap (0,0)); a tap adds the
    // uniform offset toff[t] (for the 3x3 modes the taps are sorted by (dy, dx), see make_plan, so that the offset
    // is a compile-time immediate of the ds_read)
    int apos[TMW];
#pragma unroll
    for (int tm = 0; tm < TMW; ++tm) {
        const int pidx = (wm * TMW + tm) * 32 + l31;
        apos[tm] = ((pidx >> 4) * LPWB + (pidx & 15)) * APITCH + 16 * h;
    }
    int toff[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
        toff[t] = t < ph.ntaps ? ((ph.dy[t] - p.dymin) * LPWB + (ph.dx[t] - p.dxmin)) * APITCH : 0;
    // (MERGED_S2) switch the phase-dependent state — input image, weight taps, LDS tap offsets — to parity phase q
    auto enter_phase = [&](const Phase& q) __attribute__((always_inline)) {
        xb = reinterpret_cast<const char*>(p.x) + (q.in_off + (long long)b * p.x_batch_stride) * XB;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            wtap[t] = t < q.ntaps ? q.widx[t] * cq8 * p.Cout : 0;
            toff[t] = t < q.ntaps ? ((q.dy[t] - p.dymin) * LPWB + (q.dx[t] - p.dxmin)) * APITCH : 0;
        }
    };

    f32x16 acc[TMW][TN];
#pragma unroll
    for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    constexpr PartOrder PO = kind_order(KD);
    constexpr int NPROD = PO.nprod;

    // the K loop for a compile-time tap count NT (9: 3x3, 4/2/1: the phases of the stride-2 transposed conv and
    // the 1x1 conv).  U chunks are unrolled so that U*NT is a multiple of the ring size: every item then has a
    // compile-time ring slot and the whole group is straight-line code.
    auto run = [&](auto nt_tag) __attribute__((always_inline)) {
        constexpr int NT = decltype(nt_tag)::value;
        constexpr bool EARLY_A = NT == 9;
        // ring size: divides U*NT (the single-pass fp16 mode has a third of the MFMA time per item: deeper ring)
        constexpr int RB = NT == 9 ? (NPROD == 1 ? 6 : 3) : NT == 4 ? 4 : 2;
        constexpr int U = 2;                                   // chunk pairs: chunk parity = A buffer = compile time
        u32x4 bq[RB][TN][NPB];
        // loads of item (chunk c, tap t) into ring slot `slot`; c is clamped so that the look-ahead past the last
        // chunk re-reads valid memory instead of branching
        auto issue_b = [&](int c, auto t_tag, auto slot_tag) __attribute__((always_inline)) {
            constexpr int T = decltype(t_tag)::value, SL = decltype(slot_tag)::value;
            const int cc = min(c, c_end - 1);
#pragma unroll
            for (int q = 0; q < NPB; ++q) {
                const char* base = wb + (long long)(q * part_stride + wtap[T] + cc * 2 * p.Cout) * 16;   // uniform
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) bq[SL][tn][q] = *reinterpret_cast<const u32x4*>(base + bth[tn]);
            }
        };
        u32x4 af[2][TMW][NP];                                // A fragments of the current and the next tap
        auto read_a = [&](auto u_tag, auto t_tag) __attribute__((always_inline)) {
            constexpr int UU = decltype(u_tag)::value, T = decltype(t_tag)::value;
            const char* Ac = As + UU * A_BUF;               // chunk parity = LDS buffer: immediate offsets
#pragma unroll
            for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    if constexpr (NT == 9)
                        af[T & 1][tm][q] = *reinterpret_cast<const u32x4*>(
                            Ac + q * A_PART + ((T / 3) * LPWB + T % 3) * APITCH + apos[tm]);
                    else
                        af[T & 1][tm][q] = *reinterpret_cast<const u32x4*>(Ac + q * A_PART + toff[T & 3] + apos[tm]);
                }
        };
        // The patch of chunk c+1 is converted and written to the OTHER LDS buffer inside the last A_PER_T taps of
        // chunk c, one slot per tap and in the same scheduling region as that tap's MFMAs, so that the VALU work
        // of the conversion is issued between MFMAs instead of in front of the barrier.
        auto item = [&](int c, auto u_tag, auto t_tag) __attribute__((always_inline)) {
            constexpr int UU = decltype(u_tag)::value, T = decltype(t_tag)::value;
            constexpr int SL = (UU * NT + T) % RB;
            // LDS reads of the next tap go out before this tap's MFMAs (the last tap of a chunk has no successor in
            // this buffer: the next chunk's patch is published by the barrier in between)
            // (sched_barrier: without it the scheduler sinks every load to just before its first use to save
            // registers, i.e. it undoes the look-ahead)
            if constexpr (T + 1 < NT) read_a(u_tag, std::integral_constant<int, T + 1>{});
            {   // B fragments of the item RB-1 ahead, into the slot the PREVIOUS item has just finished with: issued in
                // front of this item's MFMAs, so the youngest load at the loop's back edge (where hipcc drains vmcnt
                // to 0) is a whole item old instead of brand new
                constexpr int TE = (T + RB - 1) % NT, DCE = (T + RB - 1) / NT, SLE = (UU * NT + T + RB - 1) % RB;
                issue_b(c + DCE, std::integral_constant<int, TE>{}, std::integral_constant<int, SLE>{});
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pr = 0; pr < NPROD; ++pr)
#pragma unroll
                for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = mfma16<F16>(af[T & 1][tm][PO.pa[pr]], bq[SL][tn][PO.pb[pr]], acc[tm][tn]);
#pragma unroll
            for (int k = 0; k < A_PER_T; ++k) {
                const int tk = NT - A_PER_T + k < 0 ? 0 : NT - A_PER_T + k;      // tap that carries slot k
                if (tk == T) {
                    if (k == 0) store_a(min(c + 1, c_end - 1), std::integral_constant<int, 1 - UU>{}, std::integral_constant<int, 0>{});
                    if (k == 1) store_a(min(c + 1, c_end - 1), std::integral_constant<int, 1 - UU>{}, std::integral_constant<int, 1>{});
                    if (k == 2) store_a(min(c + 1, c_end - 1), std::integral_constant<int, 1 - UU>{}, std::integral_constant<int, 2>{});
                }
            }
            // 9 taps: the patch of chunk c+1 is fetched at the FIRST tap of chunk c and converted under its last taps, so
            // nothing but B fragments is in flight at the loop's back edge, where hipcc drains vmcnt to 0 (its wait-count
            // analysis is conservative at loop headers) — with the fetch at the last tap that drain waited for HBM.
            // Fewer taps: fetch at the last tap for chunk c+2 (a whole chunk of cover).
            if constexpr (EARLY_A) {
                if constexpr (T == 0) load_a(min(c + 1, c_end - 1));
            } else {
                if constexpr (T == NT - 1) load_a(min(c + 2, c_end - 1));
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto chunk = [&](int c, auto u_tag) __attribute__((always_inline)) {
            __syncthreads();                                // publishes the patch of chunk c
            read_a(u_tag, std::integral_constant<int, 0>{});
            __builtin_amdgcn_sched_barrier(0);
            item(c, u_tag, std::integral_constant<int, 0>{});
            if constexpr (NT > 1) item(c, u_tag, std::integral_constant<int, 1>{});
            if constexpr (NT > 2) {
                item(c, u_tag, std::integral_constant<int, 2>{});
                item(c, u_tag, std::integral_constant<int, 3>{});
            }
            if constexpr (NT > 4) {
                item(c, u_tag, std::integral_constant<int, 4>{});
                item(c, u_tag, std::integral_constant<int, 5>{});
                item(c, u_tag, std::integral_constant<int, 6>{});
                item(c, u_tag, std::integral_constant<int, 7>{});
                item(c, u_tag, std::integral_constant<int, 8>{});
            }
        };
        if (c_begin >= c_end) return;
        __syncthreads();                                    // styles are in LDS
        load_a(c_begin);
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        if constexpr (!EARLY_A) load_a(min(c_begin + 1, c_end - 1));
        // prologue: the first RB items
        issue_b(c_begin + 0 / NT, std::integral_constant<int, 0 % NT>{}, std::integral_constant<int, 0>{});
        // (the item itself issues the fragments RB-1 ahead, so the prologue stops one item short)
        constexpr int NPRO = RB - 1;
        if constexpr (NPRO > 1)
            issue_b(c_begin + 1 / NT, std::integral_constant<int, 1 % NT>{}, std::integral_constant<int, 1>{});
        if constexpr (NPRO > 2)
            issue_b(c_begin + 2 / NT, std::integral_constant<int, 2 % NT>{}, std::integral_constant<int, 2>{});
        if constexpr (NPRO > 3)
            issue_b(c_begin + 3 / NT, std::integral_constant<int, 3 % NT>{}, std::integral_constant<int, 3>{});
        if constexpr (NPRO > 4)
            issue_b(c_begin + 4 / NT, std::integral_constant<int, 4 % NT>{}, std::integral_constant<int, 4>{});
        if constexpr (NPRO > 5)
            issue_b(c_begin + 5 / NT, std::integral_constant<int, 5 % NT>{}, std::integral_constant<int, 5>{});
        static_assert((U * NT) % RB == 0, "ring slots must repeat every iteration");
        for (int cg = c_begin; cg < c_end; cg += U) {
            chunk(cg, std::integral_constant<int, 0>{});
            if (cg + 1 >= c_end) break;
            chunk(cg + 1, std::integral_constant<int, 1>{});
        }
    };
    if constexpr (MERGED_S2) {
        run(std::integral_constant<int, 4>{});            // parity (0,0): phase[0] is the state set up above
        enter_phase(p.phase[1]);
        run(std::integral_constant<int, 2>{});
        enter_phase(p.phase[2]);
        run(std::integral_constant<int, 2>{});
        enter_phase(p.phase[3]);
        run(std::integral_constant<int, 1>{});
    } else {
        run(std::integral_constant<int, NTAPS>{});
    }

    // ---- epilogue.  C/D layout of 32x32: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5): the 16 registers of
    // a tile are 2 patch rows (r>>3) x columns 8*((r>>2)&1) + 4h + (r&3).  One 64-bit row pointer per (tile, patch
    // row); everything else is a 32-bit offset (the per-element 64-bit index products were ~8k VALU cycles per wave).
    float* out = p.out + (size_t)(ks * p.nslab + ph.slab) * p.slab;       // (YH: no split-K, p.out = y as fp16)
    const int cstep = ph.sx * p.Cout;                                     // elements between neighbouring columns
    float vmax = 0.f;                                                     // max |y| of this lane's stores (y_absmax)
    // fused toRGB (hfagp.h rgb_w / rgb_part): rgbp[position][r] collects y[co] * rgb_w[r][co] over this lane's channels
    constexpr bool RGB = NTAPS == 9 || NTAPS == 1;
    const bool do_rgb = RGB && p.fused && p.rgb_part != nullptr;
    float rgbp[RGB ? TMW * 16 * 3 : 1];
    if constexpr (RGB) {
#pragma unroll
        for (int i = 0; i < TMW * 16 * 3; ++i) rgbp[i] = 0.f;
    }
    if constexpr (!ELEG) {
        // The batched form (conv16_common.h; the 32-channel loop below has the same): a lane's 32 noise values (position (tm, rw, q);
        // rows and columns past the phase's grid clamped) and, per N tile, dcoef, bias and the three rgb_w in ONE batch in front of
        // the first store; then, M tile by M tile (its accumulators are free once stored: with all 64 outputs held beside the 96
        // toRGB sums the fp16 kinds spilled), the outputs in place of their accumulators and their stores, branch-free.  The
        // arithmetic of an output and the order of the toRGB sums are the previous epilogue's: the same bits.
        constexpr int EB = YH ? 2 : 4;                                    // bytes per stored element
        unsigned co_b[TN];                                                // byte offset of the lane's channel in an fp32 vector
        bool co_ok[TN];                                                   // (Cout = 96: the last 32 columns of the tile do not exist)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int co = co0 + (wn * TN + tn) * 32 + l31;
            co_b[tn] = (unsigned)co * 4u;
            co_ok[tn] = co < p.Cout;
        }
        float nz[TMW * 16], dv[TN], bv[TN], rw3[TN][RGB ? 3 : 1];
        if (p.fused) {
            const __amdgpu_buffer_rsrc_t r_nz = epi_rsrc(p.noise, (unsigned)(p.Ho * p.Wo) * 4u);
            const __amdgpu_buffer_rsrc_t r_d = epi_rsrc(p.dcoef ? p.dcoef + (size_t)b * p.Cout : nullptr, (unsigned)p.Cout * 4u);
            const __amdgpu_buffer_rsrc_t r_b = epi_rsrc(p.bias, (unsigned)p.Cout * 4u);
            const __amdgpu_buffer_rsrc_t r_w = epi_rsrc(do_rgb ? p.rgb_w + (size_t)b * 3 * p.Cout : nullptr, (unsigned)(3 * p.Cout) * 4u);
#pragma unroll
            for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
                for (int rw = 0; rw < 2; ++rw) {
                    const int oy = ph.sy * min(m0 + 2 * (wm * TMW + tm) + rw, ph.mh - 1) + ph.oy0;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int n = min(n0 + 8 * (q >> 2) + 4 * h + (q & 3), ph.mw - 1);
                        nz[(tm * 2 + rw) * 8 + q] = epi_load(r_nz, (unsigned)(oy * p.Wo + ph.ox0 + ph.sx * n) * 4u);
                    }
                }
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {                             // (a channel past Cout is past these resources: 0)
                dv[tn] = epi_load(r_d, co_b[tn]);
                bv[tn] = epi_load(r_b, co_b[tn]);
                if constexpr (RGB) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) rw3[tn][c] = epi_load(r_w, (unsigned)(c * p.Cout) * 4u + co_b[tn]);
                }
            }
#pragma unroll
            for (int i = 0; i < TMW * 16; ++i) epi_landed(nz[i]);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                epi_landed(dv[tn]);
                epi_landed(bv[tn]);
                if constexpr (RGB) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) epi_landed(rw3[tn][c]);
                }
            }
#pragma unroll
            for (int i = 0; i < TMW * 16; ++i) nz[i] = p.noise ? nz[i] * p.noise_strength : 0.f;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) dv[tn] = p.dcoef ? dv[tn] * sback : sback;
        }
        // the stores go through a resource that starts at the tile's first output element (row sy m0 + oy0, column ox0 of sample b)
        // and ends with the tile's rows or with the image: an element outside the grid or past Cout gets EPI_OOB
        const int oyb = ph.sy * m0 + ph.oy0;
        const unsigned pix_b = (unsigned)p.Cout * EB, row_b = (unsigned)p.Wo * pix_b;
        char* base = (YH ? reinterpret_cast<char*>(p.out) : reinterpret_cast<char*>(out)) + (((size_t)b * p.Ho + oyb) * p.Wo + ph.ox0) * pix_b;
        const __amdgpu_buffer_rsrc_t r_y = epi_rsrc(p.out ? base : nullptr, (unsigned)min((p.Ho - oyb) * p.Wo - ph.ox0, ph.sy * PH * p.Wo) * pix_b);
#pragma unroll
        for (int tm = 0; tm < TMW; ++tm) {
            if (p.fused) {
                // an element outside the grid or past Cout counts for nothing in vmax; a channel past Cout adds nothing to the toRGB
                // sums (the sums of a position outside the grid are never written)
#pragma unroll
                for (int rw = 0; rw < 2; ++rw) {
                    const bool row_ok = m0 + 2 * (wm * TMW + tm) + rw < ph.mh;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const bool ok = row_ok && n0 + 8 * (q >> 2) + 4 * h + (q & 3) < ph.mw;
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn) {
                            const float v = lrelu_gain_clamp(acc[tm][tn][8 * rw + q] * dv[tn] + bv[tn] + nz[(tm * 2 + rw) * 8 + q], p.act,
                                                             p.alpha, p.gain, p.clamp);
                            acc[tm][tn][8 * rw + q] = v;
                            vmax = fmaxf(vmax, ok && co_ok[tn] ? fabsf(v) : 0.f);
                            if constexpr (RGB) {
                                const float vc = co_ok[tn] ? v : 0.f;
#pragma unroll
                                for (int c = 0; c < 3; ++c)
                                    rgbp[((tm * 2 + rw) * 8 + q) * 3 + c] = fmaf(vc, rw3[tn][c], rgbp[((tm * 2 + rw) * 8 + q) * 3 + c]);
                            }
                        }
                    }
                }
            } else if constexpr (F16) {
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[tm][tn][r] *= sback;      // (element by element: no packed fp32, build.sh)
            }
            if (p.out) {                     // (NULL: the caller only wants the fused toRGB sums — last SR layer, forward only)
#pragma unroll
                for (int rw = 0; rw < 2; ++rw) {
                    const int mr = 2 * (wm * TMW + tm) + rw;                 // row of the tile
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int n = n0 + 8 * (q >> 2) + 4 * h + (q & 3);
                        const bool ok = m0 + mr < ph.mh && n < ph.mw;
                        const unsigned pos_b = (unsigned)(ph.sy * mr) * row_b + (unsigned)(ph.sx * n) * pix_b;
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn) {
                            const unsigned off = ok && co_ok[tn] ? pos_b + (co_b[tn] >> 2) * EB : EPI_OOB;
                            if constexpr (YH)
                                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(short, (_Float16)acc[tm][tn][8 * rw + q]), r_y, off, 0, 0);
                            else
                                epi_store(r_y, off, acc[tm][tn][8 * rw + q]);
                        }
                    }
                }
            }
        }
        if (p.fused && p.y_absmax) publish_absmax(p.y_absmax, vmax, blockIdx.x * 4 + wave);
    }
    if constexpr (ELEG) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int co = co0 + (wn * TN + tn) * 32 + l31;
        if (co >= p.Cout) continue;
        float rw3[3] = {0.f, 0.f, 0.f};
        if constexpr (RGB)
            if (do_rgb) {
#pragma unroll
                for (int r = 0; r < 3; ++r) rw3[r] = p.rgb_w[((size_t)b * 3 + r) * p.Cout + co];
            }
        float d = sback, bs = 0.f;
        if (p.fused) {
            if (p.dcoef) d = p.dcoef[(size_t)b * p.Cout + co] * sback;
            if (p.bias) bs = p.bias[co];
        }
#pragma unroll
        for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
            for (int rw = 0; rw < 2; ++rw) {
                const int m = m0 + 2 * (wm * TMW + tm) + rw;
                if (m >= ph.mh) continue;
                const int oy = ph.sy * m + ph.oy0;
                const size_t rowoff = (((size_t)b * p.Ho + oy) * p.Wo + ph.ox0) * p.Cout + co;
                float* rowp = out + rowoff;
                _Float16* rowh = reinterpret_cast<_Float16*>(p.out) + rowoff;
                const float* nrow = (p.fused && p.noise) ? p.noise + (size_t)oy * p.Wo + ph.ox0 : nullptr;
                float nz[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int n = min(n0 + 8 * (q >> 2) + 4 * h + (q & 3), ph.mw - 1);
                    nz[q] = nrow ? nrow[ph.sx * n] * p.noise_strength : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int n = n0 + 8 * (q >> 2) + 4 * h + (q & 3);
                    if (n >= ph.mw) continue;
                    float v = acc[tm][tn][8 * rw + q];
                    if (p.fused) v = lrelu_gain_clamp(v * d + bs + nz[q], p.act, p.alpha, p.gain, p.clamp);
                    else if constexpr (F16) v *= sback;
                    vmax = fmaxf(vmax, fabsf(v));
                    if (p.out) {                 // (NULL: the caller only wants the fused toRGB sums — last SR layer, forward only)
                        if constexpr (YH) rowh[n * cstep] = (_Float16)v;
                        else rowp[n * cstep] = v;
                    }
                    if constexpr (RGB) {
#pragma unroll
                        for (int r = 0; r < 3; ++r)
                            rgbp[((tm * 2 + rw) * 8 + q) * 3 + r] = fmaf(v, rw3[r], rgbp[((tm * 2 + rw) * 8 + q) * 3 + r]);
                    }
                }
            }
    }
    if (p.fused && p.y_absmax) publish_absmax(p.y_absmax, vmax, blockIdx.x * 4 + wave);
    }   // ELEG
    if constexpr (RGB) {
        if (do_rgb) {
            // reduce-scatter over the 32 channel lanes: at the step with lane bit m the lane keeps one half of its values
            // and adds the partner's copy of that half; after 5 steps lane l31 owns the 3 sums of position l31
            // (position index = (tm*2 + rw)*8 + q, exactly the order of rgbp): 93 exchanges instead of 5 x 96
            int n = TMW * 16 * 3;
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) {
                n >>= 1;
                const bool up = (l31 & m) != 0;
#pragma unroll
                for (int i = 0; i < TMW * 16 * 3 / 2; ++i) {
                    if (i < n) {
                        const float keep = up ? rgbp[i + n] : rgbp[i];
                        const float give = up ? rgbp[i] : rgbp[i + n];
                        rgbp[i] = keep + __shfl_xor(give, m);
                    }
                }
            }
            const int pos = l31;                                  // (tm*2 + rw)*8 + q
            const int tm = pos >> 4, rw = (pos >> 3) & 1, q = pos & 7;
            const int m = m0 + 2 * (wm * TMW + tm) + rw, nn = n0 + 8 * (q >> 2) + 4 * h + (q & 3);
            if (m < ph.mh && nn < ph.mw) {
                const int part = tn_blk * WN + wn;
                float4* dst = reinterpret_cast<float4*>(p.rgb_part) +
                              (((size_t)part * p.B + b) * p.Ho + (ph.sy * m + ph.oy0)) * p.Wo + (ph.sx * nn + ph.ox0);
                *dst = make_float4(rgbp[0], rgbp[1], rgbp[2], 0.f);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The stride-2 transposed 3x3 convolution (mode CONVT3X3_UP2) with its four output phases MERGED in one block:
// the input patch of a K chunk is staged once and its 4+2+2+1 = 9 taps feed four accumulator sets (one per output
// parity), instead of four passes that each re-stage the patch for 4, 2, 2 and 1 taps.  M = 8x16 input positions,
// N = 64 output channels per block (4 phases x 2 x 1 MFMA tiles per wave = 128 accumulator registers).
// The taps are grouped by their LDS shift (dy, dx) so that each shifted A fragment is read once per chunk:
//   shift ( 0, 0): phase 0 w[0], phase 1 w[1], phase 2 w[3], phase 3 w[4]
//   shift (-1, 0): phase 0 w[6], phase 1 w[7]        shift (0,-1): phase 0 w[2], phase 2 w[5]
//   shift (-1,-1): phase 0 w[8]                       (w[k] = tap k of the 3x3 kernel, y_t[2i+ti][2j+tj] += x[i][j] w[ti][tj])
// NW = 4 waves: N = 64 channels per block, one wave per SIMD.  NW = 8 waves (2 x 4 wave grid, 512 threads): N = 128
// channels per block and two waves per SIMD (256 registers each) — the patch is staged once for twice the MFMA
// work and the second wave of a SIMD covers the barrier / staging bubbles of the first; used when the layer
// still fills the chip with the larger tile (make_plan).
constexpr int UP4_OCC = 2;          // blocks per CU the 4-wave variant is compiled for (128 accumulators + 128 registers)
template <int KD, int NW, int IO = 0>
__global__ void __launch_bounds__(NW * 64, (NW == 4 && KD != 3) ? UP4_OCC : 1) upconv_bf16_kernel(const ConvParams p) {
    constexpr int NP = kind_parts_a(KD), NPB = kind_parts(KD);    // parts of the activations (LDS patch) / of the weight image
    constexpr bool F16 = kind_f16(KD);
    constexpr bool XH = (IO & 1) != 0, YH = (IO & 2) != 0;       // fp16 storage of x / y_t (see modconv_bf16_kernel)
    constexpr int XB = XH ? 2 : 4;
    static_assert(IO == 0 || KD == 1, "fp16 storage goes with the single-pass fp16 arithmetic");
    constexpr int NTH = NW * 64;
    constexpr int TM = 2, TN = 1, WN = NW / 2, BM = 128, BNU = WN * TN * 32, PH = BM / PW, RB = kind_nprod(KD) == 1 ? 6 : 3;
    constexpr int LPWB = RowPitch<NP>::value;
    constexpr int APOS = (PH + 2) * LPWB;
    constexpr int A_PART = APOS * APITCH, A_BUF = NP * A_PART;
    using namespace up_items;
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    char* As = lds_raw;
    float* Ss = reinterpret_cast<float*>(lds_raw + 2 * A_BUF);

    // ---- tiling (round 6).  The position grid of the even parity is (H+1) x (W+1): tiling it per sample in 8 x 16 tiles rounds BOTH
    // extents up (257 -> 33 x 17 tiles instead of 32 x 16: 1.10 x the MFMA work at 256^2, 1.41 x at 64^2, 1.88 x at 32^2).  Now:
    //   * the rows of all samples are STACKED with pitch RP = H+1 (row r = b RP + m; row m = H of a sample is the zero padding
    //     below its image, which is also what the tap (-1, .) of row 0 of the next sample has to see): B (H+1) rows tile in 8s
    //     without a remainder per sample; a tile may straddle samples (styles / range-guard scales of up to `up_ns` samples);
    //   * the columns 0 .. W-1 are tiled in 16s exactly (W % 16 == 0) and the one remaining column n = W (only x[.][W-1] reaches
    //     it: taps (0,-1), (-1,-1)) goes to FRINGE tiles: the same 8 x 16 tile and K loop, but tile column j stands for
    //     (row block j >> 1, image column W-1 + (j & 1)) — eight two-column pieces of eight different 8-row blocks, of which the odd
    //     columns are stored.  64 useful positions per fringe tile; B (H+1) / 64 of them per layer (0.8 % of the tiles at 256^2).
    unsigned id = p.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tiles_nu = p.Cout / BNU;
    const int tn_blk = __builtin_amdgcn_readfirstlane(id % tiles_nu);  id /= tiles_nu;
    const int n_reg = p.up_tr * p.up_tw, n_tile = n_reg + p.up_nf;
    const int T = __builtin_amdgcn_readfirstlane(id % n_tile);         id /= n_tile;
    const int ks = __builtin_amdgcn_readfirstlane(id);
    const bool fringe = T >= n_reg;                                    // block-uniform
    const int RP = p.up_rp, R_total = p.up_rows;
    // regular tile: rows r0 .. r0+7, columns n0 .. n0+15; fringe tile: rows r0 .. r0+63
    const int r0 = fringe ? (T - n_reg) * 64 : (T / p.up_tw) * PH, n0 = fringe ? 0 : (T % p.up_tw) * PW;
    const int co0 = tn_blk * BNU;
    const int b_lo = min(max(r0 - 1, 0) / RP, p.B - 1);                // first sample the patch touches

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int h = lane >> 5, l31 = lane & 31;
    const int c_begin = __builtin_amdgcn_readfirstlane((int)(((long long)p.nchunks * ks) / p.ksplit));
    const int c_end = __builtin_amdgcn_readfirstlane((int)(((long long)p.nchunks * (ks + 1)) / p.ksplit));

    // ---- A staging (as in modconv_bf16_kernel): patch rows r0-1 .. r0+PH-1, columns n0-1 .. n0+PW-1 (fringe: see above)
    const int npatch = p.ph * p.pw;
    constexpr int A_PER_T = ((PH + 2) * (PW + 2) * 4 + NTH - 1) / NTH;
    static_assert(A_PER_T == 2 || A_PER_T == 3, "staging schedule: two or three slots per thread");
    float4 ra[A_PER_T];
    const char* xb = reinterpret_cast<const char*>(p.x) + (long long)b_lo * p.x_batch_stride * XB;
    // styles of the up_ns samples from b_lo on (ones past the batch), then the fp16 range-guard scales 2^-e | 2^e per sample
    float* Gd = Ss + p.up_ns * p.Cin;                              // [up_ns] 2^-e, then [up_ns] 2^e
    {
        const long long s_lo = (long long)b_lo * p.Cin, s_n = (long long)p.B * p.Cin;
        for (int i = tid; i < p.up_ns * p.Cin; i += NTH) Ss[i] = (p.styles && s_lo + i < s_n) ? p.styles[s_lo + i] : 1.f;
        for (int sI = 0; sI < p.up_ns; ++sI) {
            float bk = 1.f, dn = 1.f;
            if constexpr (F16)
                dn = style_range_guard((p.styles && b_lo + sI < p.B) ? p.styles + (size_t)(b_lo + sI) * p.Cin : nullptr, p.Cin, lane, &bk,
                                       p.x_absmax, p.w_absmax);
            if (tid == 0) { Gd[sI] = dn; Gd[p.up_ns + sI] = bk; }
        }
    }
    __syncthreads();
    unsigned aoff[A_PER_T];
    int lds_a[A_PER_T], soff[A_PER_T];
    float amask[A_PER_T];
#pragma unroll
    for (int k = 0; k < A_PER_T; ++k) {
        const int idx = min(tid + k * NTH, npatch * 4 - 1);
        const int pix = idx >> 2, q = idx & 3;
        const int pi = pix / p.pw, pj = pix % p.pw;
        lds_a[k] = (pi * LPWB + pj) * APITCH + 8 * q;
        int r, n;
        if (!fringe) { r = r0 - 1 + pi; n = n0 - 1 + pj; }
        else { r = pj == 0 ? -1 : r0 + 8 * ((pj - 1) >> 1) + pi - 1; n = p.W - 1 + ((pj - 1) & 1); }
        const bool row_ok = r >= 0 && r < R_total;
        const int bb = row_ok ? r / RP : b_lo, m = r - bb * RP;
        const bool inside = row_ok && m < p.H && n >= 0 && n < p.W;
        const int sel = inside ? bb - b_lo : 0;
        aoff[k] = inside ? (unsigned)(((long long)sel * p.x_batch_stride + (long long)(m * p.W + n) * p.Cin + 4 * q) * XB) : 0u;
        amask[k] = inside ? Gd[sel] : 0.f;          // zero padding and the fp16 range guard in one factor
        soff[k] = sel * p.Cin + 4 * q;
    }
    auto load_a = [&](int chunk) __attribute__((always_inline)) { a16_load<XH>(ra, xb, chunk, aoff); };
    auto store_a = [&](int chunk, auto buf_tag, auto k_tag) __attribute__((always_inline)) {
        constexpr int BUF = decltype(buf_tag)::value, k = decltype(k_tag)::value;
        a16_store<KD, XH>(As + BUF * A_BUF, A_PART, lds_a[k], amask[k], *reinterpret_cast<const float4*>(Ss + chunk * CKB + soff[k]), ra[k]);
    };

    // ---- B fragments: one 32-column tile per wave, ring of RB items
    const char* wb = reinterpret_cast<const char*>(p.wt);
    const int cq8 = p.Cin >> 3;
    const int part_stride = 9 * cq8 * p.Cout;
    unsigned bth[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) bth[tn] = (unsigned)(h * p.Cout + co0 + (wn * TN + tn) * 32 + l31) * 16u;
    int apos[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int pidx = (wm * TM + tm) * 32 + l31;
        apos[tm] = ((pidx >> 4) * LPWB + (pidx & 15)) * APITCH + 16 * h;
    }

    f32x16 acc[4][TM][TN];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[f][tm][tn][r] = 0.f;

    constexpr PartOrder PO = kind_order(KD);
    constexpr int NPROD = PO.nprod;
    u32x4 bq[RB][TN][NPB];
    u32x4 af[2][TM][NP];                  // A fragments of the current and the next shift group
    auto issue_b = [&](int c, auto i_tag, auto slot_tag) __attribute__((always_inline)) {
        constexpr int I = decltype(i_tag)::value, SL = decltype(slot_tag)::value;
        const int cc = min(c, c_end - 1);
#pragma unroll
        for (int q = 0; q < NPB; ++q) {
            const char* base = wb + (long long)(q * part_stride + (I_W[I] * cq8 + cc * 2) * p.Cout) * 16;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bq[SL][tn][q] = *reinterpret_cast<const u32x4*>(base + bth[tn]);
        }
    };
    auto read_a = [&](auto u_tag, auto g_tag) __attribute__((always_inline)) {
        constexpr int UU = decltype(u_tag)::value, G = decltype(g_tag)::value;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int q = 0; q < NP; ++q)
                af[G & 1][tm][q] = *reinterpret_cast<const u32x4*>(As + UU * A_BUF + q * A_PART + group_pos(G, LPWB) * APITCH + apos[tm]);
    };
    auto item = [&](int c, auto u_tag, auto i_tag) __attribute__((always_inline)) {
        constexpr int I = decltype(i_tag)::value, G = I_GRP[I], F = I_PHASE[I];
        constexpr int SL = (decltype(u_tag)::value * NITEM + I) % RB;     // ring slot: repeats every chunk pair
        if constexpr (I == G_FIRST[G] && G < 3) read_a(u_tag, std::integral_constant<int, G + 1>{});
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pr = 0; pr < NPROD; ++pr)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[F][tm][tn] = mfma16<F16>(af[G & 1][tm][PO.pa[pr]], bq[SL][tn][PO.pb[pr]], acc[F][tm][tn]);
        // the patch of the next chunk is converted into the other LDS buffer under the last A_PER_T items
        if constexpr (I >= NITEM - A_PER_T)
            store_a(min(c + 1, c_end - 1), std::integral_constant<int, 1 - decltype(u_tag)::value>{},
                    std::integral_constant<int, I - (NITEM - A_PER_T)>{});
        issue_b(c + (I + RB) / NITEM, std::integral_constant<int, (I + RB) % NITEM>{}, std::integral_constant<int, SL>{});
        if constexpr (I == NITEM - 1) load_a(min(c + 2, c_end - 1));
        __builtin_amdgcn_sched_barrier(0);
    };
    auto chunk = [&](int c, auto u_tag) __attribute__((always_inline)) {
        __syncthreads();                                    // publishes the patch of chunk c
        read_a(u_tag, std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        item(c, u_tag, std::integral_constant<int, 0>{});
        item(c, u_tag, std::integral_constant<int, 1>{});
        item(c, u_tag, std::integral_constant<int, 2>{});
        item(c, u_tag, std::integral_constant<int, 3>{});
        item(c, u_tag, std::integral_constant<int, 4>{});
        item(c, u_tag, std::integral_constant<int, 5>{});
        item(c, u_tag, std::integral_constant<int, 6>{});
        item(c, u_tag, std::integral_constant<int, 7>{});
        item(c, u_tag, std::integral_constant<int, 8>{});
    };
    static_assert((2 * NITEM) % RB == 0 && RB <= NITEM, "ring slots must repeat every chunk pair");
    if (c_begin < c_end) {
        __syncthreads();                                    // styles are in LDS
        load_a(c_begin);
        issue_b(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        issue_b(c_begin, std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
        issue_b(c_begin, std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
        if constexpr (RB > 3) {
            issue_b(c_begin, std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{});
            issue_b(c_begin, std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{});
            issue_b(c_begin, std::integral_constant<int, 5>{}, std::integral_constant<int, 5>{});
        }
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        if constexpr (A_PER_T > 2) store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        load_a(min(c_begin + 1, c_end - 1));
        // pairs of chunks (LDS buffer = chunk parity = compile time), then the odd one: an exit in the MIDDLE of the
        // loop body made the register allocator keep the 128 accumulators in two AGPR sets and copy them
        // (~190 v_accvgpr_mov per 108 MFMAs)
        int cg = c_begin;
        for (; cg + 1 < c_end; cg += 2) {
            chunk(cg, std::integral_constant<int, 0>{});
            chunk(cg + 1, std::integral_constant<int, 1>{});
        }
        if (cg < c_end) chunk(cg, std::integral_constant<int, 0>{});
    }

    // ---- raw stores of the four phases: y_t[2m + (f>>1)][2n + (f&1)], extents (H+1-(f>>1)) x (W+1-(f&1));
    // one 64-bit row pointer per (phase, tile, patch row), 32-bit column offsets
    float* out = p.out + (size_t)ks * p.slab;
    if (!fringe) {
        // the four patch rows of this wave (wave-uniform): sample, image row, range-guard scale
        int rb[2 * TM], rm[2 * TM];
        float rs[2 * TM];
#pragma unroll
        for (int i = 0; i < 2 * TM; ++i) {
            const int r = r0 + 2 * (wm * TM + (i >> 1)) + (i & 1);
            const bool ok = r < R_total;
            rb[i] = ok ? r / RP : 0;
            rm[i] = ok ? r - rb[i] * RP : (1 << 30);
            rs[i] = F16 ? Gd[p.up_ns + min(max(rb[i] - b_lo, 0), p.up_ns - 1)] : 1.f;
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int mh = p.H + 1 - (f >> 1), mw = p.W + 1 - (f & 1);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int co = co0 + (wn * TN + tn) * 32 + l31;
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int rw = 0; rw < 2; ++rw) {
                        const int m = rm[2 * tm + rw];
                        if (m >= mh) continue;
                        const size_t rowoff = (((size_t)rb[2 * tm + rw] * p.Ho + 2 * m + (f >> 1)) * p.Wo + (f & 1)) * p.Cout + co;
                        float* rowp = out + rowoff;
                        _Float16* rowh = reinterpret_cast<_Float16*>(p.out) + rowoff;
                        const float sb = rs[2 * tm + rw];
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const int n = n0 + 8 * (q >> 2) + 4 * h + (q & 3);
                            if (n >= mw) continue;
                            {
                                const float v = F16 ? acc[f][tm][tn][8 * rw + q] * sb : acc[f][tm][tn][8 * rw + q];
                                if constexpr (YH) rowh[2 * n * p.Cout] = (_Float16)v;
                                else rowp[2 * n * p.Cout] = v;
                            }
                        }
                    }
            }
        }
    } else {
        // fringe tile: tile column j = 8 (q >> 2) + 4 h + (q & 3) is odd exactly for odd q; it is image column W of row
        // r0 + 8 (j >> 1) + patch row -> y_t[2m + fy][2W] of the two even-column parities (f = 0, 2)
#pragma unroll
        for (int f = 0; f < 4; f += 2) {
            const int mh = p.H + 1 - (f >> 1);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int co = co0 + (wn * TN + tn) * 32 + l31;
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int rw = 0; rw < 2; ++rw)
#pragma unroll
                        for (int q = 1; q < 8; q += 2) {
                            const int j = 8 * (q >> 2) + 4 * h + (q & 3);
                            const int r = r0 + 8 * (j >> 1) + 2 * (wm * TM + tm) + rw;
                            if (r >= R_total) continue;
                            const int bb = r / RP, m = r - bb * RP;
                            if (m >= mh) continue;
                            const size_t off = (((size_t)bb * p.Ho + 2 * m + (f >> 1)) * p.Wo + 2 * p.W) * p.Cout + co;
                            const float v = F16 ? acc[f][tm][tn][8 * rw + q] * Gd[p.up_ns + min(bb - b_lo, p.up_ns - 1)]
                                                : acc[f][tm][tn][8 * rw + q];
                            if constexpr (YH) reinterpret_cast<_Float16*>(p.out)[off] = (_Float16)v;
                            else out[off] = v;
                        }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The forward 3x3 conv at F16X3 (KD = 4) on v_mfma_f32_16x16x32_f16 with 32-channel K chunks (modconv_bf16_kernel<4, 2, 9, 0, 1>;
// make_plan / launch_group pick it for mode CONV3X3 at F16X3 with fp32 storage, Cin % 32 == 0 and Cout % 128 == 0).
//   * Same block tile (8 x 16 positions x 128 channels, 4 waves of 64 positions x 64 channels), same split operands (the A parts
//     are bit for bit those of the 16-channel loop), same weight image: lane group g = lane >> 4 of a 16x16x32 B fragment reads
//     Cin octet 4 chunk + g of 16 consecutive Cout (256-B runs of [part][tap][Cin/8][Cout][8]).
//   * B fragments by buffer loads: SGPR resource, one per-lane offset for the whole kernel, tap / chunk / part in the scalar
//     offset and the N tile in the instruction's immediate: no 64-bit address arithmetic on the vector ALU.
//   * Patch image per part [channel octet][position][16 B] (octet stride 3072 B = 0 mod 256 B): the 16 lanes of each
//     ds_read_b128 group read 16 consecutive 16-B slots, the 16 lanes of each ds_write_b64 group 128 contiguous bytes.  Zero
//     padding comes from out-of-range buffer loads of the activations (no mask multiply), the range-guard scale 2^-e is
//     folded into the styles once.
//   * One barrier per 32 channels (432 MFMAs), B ring of two items, the A fragments of the next tap read per M tile as soon
//     as the current tap's MFMAs of that tile are issued.
namespace c9 {
constexpr int CK = 32;                            // channels per K chunk
constexpr int LP = PW + 2, NPOS = (8 + 2) * LP;   // patch row pitch / positions (10 x 18)
constexpr int OCT = 3072;                         // bytes per channel octet of one part: NPOS x 16 B rounded up to 256 B
constexpr int A_PART = 4 * OCT, A_BUF = 2 * A_PART;
constexpr int A_PER_T = 6;                        // float4 slots per thread: 180 positions x 8 quads over 256 threads
static_assert(NPOS * 16 <= OCT && OCT % 256 == 0 && NPOS * 8 <= A_PER_T * 256, "patch layout");
constexpr size_t lds_bytes(int cin) { return (size_t)2 * A_BUF + (size_t)(cin + 8) * sizeof(float); }
}  // namespace c9

template <int KD, int TM, int NTAPS, int IO, int LOOP>
__global__ void __launch_bounds__(256, 2) modconv_bf16_kernel(const ConvParams p, const int) {
    static_assert(KD == 4 && TM == 2 && NTAPS == 9 && IO == 0 && (LOOP == 1 || LOOP == 3), "the 32-channel loop is the F16X3 forward 3x3 conv");
    // LOOP = 3: the same kernel with the epilogue it had before its loads were batched (developer switch
    // HFAGP_DEV_CONV_EPILOGUE_LEGACY=1, launch_modconv_bf16): each output's operands fetched between the stores
    constexpr bool LEGACY = LOOP == 3;
    using namespace c9;
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    char* As = lds_raw;                                                // [2][2 parts][4 octets][OCT]
    float* Ss = reinterpret_cast<float*>(lds_raw + 2 * A_BUF);         // [Cin] styles x 2^-e

    unsigned id = p.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tn_blk = __builtin_amdgcn_readfirstlane(id % p.tiles_n); id /= p.tiles_n;
    const int tw = __builtin_amdgcn_readfirstlane(id % p.tiles_w);     id /= p.tiles_w;
    const int th = __builtin_amdgcn_readfirstlane(id % p.tiles_h);     id /= p.tiles_h;
    const int b = __builtin_amdgcn_readfirstlane(id % p.B);            id /= p.B;
    const int ks = __builtin_amdgcn_readfirstlane(id);
    const int m0 = th * 8, n0 = tw * PW, co0 = tn_blk * BNB;
    if (m0 >= p.Ho || n0 >= p.Wo) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int g = lane >> 4, i16 = lane & 15;
    const int nch = p.Cin / CK;
    const int c_begin = __builtin_amdgcn_readfirstlane((int)(((long long)nch * ks) / p.ksplit));
    const int c_end = __builtin_amdgcn_readfirstlane((int)(((long long)nch * (ks + 1)) / p.ksplit));

    float sback = 1.f;
    const float sdown = style_range_guard(p.styles ? p.styles + (size_t)b * p.Cin : nullptr, p.Cin, lane, &sback, p.x_absmax, p.w_absmax);
    for (int i = tid; i < p.Cin; i += 256) Ss[i] = (p.styles ? p.styles[(size_t)b * p.Cin + i] : 1.f) * sdown;

    // ---- A staging: slot e = tid + 256 k holds channels 4q .. 4q+3 (q = 2 ((e >> 4) & 3) + (e & 1)) of patch position
    // 8 (e >> 6) + ((e >> 1) & 7); q does not depend on k.  Positions past the patch repeat the last one (same value, same address).
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x + (long long)b * p.x_batch_stride), 0, (unsigned)(p.in_h * p.in_w * p.Cin) * 4u, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;                              // beyond any image: the load returns zeros
    const int qa = 2 * ((tid >> 4) & 3) + (tid & 1);
    unsigned aoff[A_PER_T];
    int lds_a[A_PER_T];
#pragma unroll
    for (int k = 0; k < A_PER_T; ++k) {
        const int pix = min(8 * ((tid >> 6) + 4 * k) + ((tid >> 1) & 7), NPOS - 1);
        lds_a[k] = (qa >> 1) * OCT + pix * 16 + (qa & 1) * 8;
        const int iy = m0 - 1 + pix / LP, ix = n0 - 1 + pix % LP;
        const bool inside = iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w;
        aoff[k] = inside ? (unsigned)((iy * p.in_w + ix) * p.Cin + 4 * qa) * 4u : OOB;
    }
    // (in two halves of three slots: 12 staging registers instead of 24)
    float4 ra[A_PER_T / 2];
    auto load_a = [&](int chunk, auto half_tag) __attribute__((always_inline)) {
        constexpr int HF = decltype(half_tag)::value;
#pragma unroll
        for (int k = 0; k < A_PER_T / 2; ++k)
            ra[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, aoff[HF * 3 + k], chunk * CK * 4, 0));
    };
    auto store_a = [&](int chunk, auto buf_tag, auto k_tag) __attribute__((always_inline)) {
        constexpr int BUF = decltype(buf_tag)::value, k = decltype(k_tag)::value;
        const float4 sv = *reinterpret_cast<const float4*>(Ss + chunk * CK + 4 * qa);
        const float4 x = ra[k % 3];
        uint2 parts[2];
        split4<KD>(make_float4(x.x * sv.x, x.y * sv.y, x.z * sv.z, x.w * sv.w), parts);
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<uint2*>(As + BUF * A_BUF + q * A_PART + lds_a[k]) = parts[q];
    };

    // ---- B fragments: [part][tap][Cin/8][Cout][8] by buffer loads; lane offset (g Cout + co) x 16, N tile tn at +256 tn
    const int cq8 = p.Cin >> 3;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.wt), 0, (unsigned)(2 * 9 * cq8 * p.Cout) * 16u, 0x00020000);
    const unsigned boff = (unsigned)(g * p.Cout + co0 + wn * 64 + i16) * 16u;
    const int part_bytes = 9 * cq8 * p.Cout * 16, tap_bytes = cq8 * p.Cout * 16, chunk_bytes = 4 * p.Cout * 16;
    // A fragment of M tile tm (patch row 4 wm + tm + dy, column i16 + dx), lane group g = channel octet g
    const int abase = g * OCT + (4 * wm * LP + i16) * 16;

    f32x4v acc[4][4];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = f32x4v{0.f, 0.f, 0.f, 0.f};

    constexpr PartOrder PO = kind_order(KD);
    u32x4 bq[2][4][2];                                                 // ring slot, N tile, part
    u32x4 af[4][2];                                                    // M tile, part (of the tap being computed)
    auto issue_b = [&](int c, int t, auto slot_tag) __attribute__((always_inline)) {
        constexpr int SL = decltype(slot_tag)::value;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int so = q * part_bytes + t * tap_bytes + c * chunk_bytes;   // scalar
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) bq[SL][tn][q] = __builtin_amdgcn_raw_buffer_load_b128(rw, boff + 256 * tn, so, 0);
        }
    };
    auto read_a = [&](auto u_tag, auto t_tag, auto tm_tag) __attribute__((always_inline)) {
        constexpr int UU = decltype(u_tag)::value, T = decltype(t_tag)::value, TMI = decltype(tm_tag)::value;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            af[TMI][q] = *reinterpret_cast<const u32x4*>(As + UU * A_BUF + q * A_PART + ((TMI + T / 3) * LP + T % 3) * 16 + abase);
    };
    auto mfma_tile = [&](auto t_tag, auto tm_tag, auto sl_tag) __attribute__((always_inline)) {
        constexpr int TMI = decltype(tm_tag)::value, SL = decltype(sl_tag)::value;
#pragma unroll
        for (int pr = 0; pr < 3; ++pr)
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
                acc[TMI][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, af[TMI][PO.pa[pr]]),
                                                                     __builtin_bit_cast(f16x8, bq[SL][tn][PO.pb[pr]]), acc[TMI][tn], 0, 0, 0);
    };
    // item = tap T of chunk c: B of the next item into the other ring slot, then per M tile its 12 MFMAs followed by the
    // reads of that tile's fragments for tap T+1; the patch of chunk c+1 is fetched in two halves (at taps 0 and 4) and
    // converted one slot per tap into the other LDS buffer under taps 2, 3, 4 and 6, 7, 8
    auto item = [&](int c, auto u_tag, auto t_tag) __attribute__((always_inline)) {
        constexpr int UU = decltype(u_tag)::value, T = decltype(t_tag)::value;
        constexpr int SL = (UU * 9 + T) & 1;
        issue_b(c + (T + 1) / 9, (T + 1) % 9, std::integral_constant<int, SL ^ 1>{});
        if constexpr (T == 0) load_a(min(c + 1, c_end - 1), std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        auto tile = [&](auto tm_tag) __attribute__((always_inline)) {
            mfma_tile(t_tag, tm_tag, std::integral_constant<int, SL>{});
            if constexpr (T + 1 < 9) read_a(u_tag, std::integral_constant<int, T + 1>{}, tm_tag);
            if constexpr ((T >= 2 && T <= 4) || T >= 6) {     // (nested: a tap without a slot must not instantiate store_a)
                if constexpr (decltype(tm_tag)::value == 3)
                    store_a(min(c + 1, c_end - 1), std::integral_constant<int, 1 - UU>{}, std::integral_constant<int, (T <= 4 ? T - 2 : T - 3)>{});
            }
            if constexpr (decltype(tm_tag)::value == 3 && T == 4) load_a(min(c + 1, c_end - 1), std::integral_constant<int, 1>{});
            __builtin_amdgcn_sched_barrier(0);
        };
        tile(std::integral_constant<int, 0>{});
        tile(std::integral_constant<int, 1>{});
        tile(std::integral_constant<int, 2>{});
        tile(std::integral_constant<int, 3>{});
    };
    auto chunk = [&](int c, auto u_tag) __attribute__((always_inline)) {
        __syncthreads();                                               // publishes the patch of chunk c
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
        __builtin_amdgcn_sched_barrier(0);
        item(c, u_tag, std::integral_constant<int, 0>{});
        item(c, u_tag, std::integral_constant<int, 1>{});
        item(c, u_tag, std::integral_constant<int, 2>{});
        item(c, u_tag, std::integral_constant<int, 3>{});
        item(c, u_tag, std::integral_constant<int, 4>{});
        item(c, u_tag, std::integral_constant<int, 5>{});
        item(c, u_tag, std::integral_constant<int, 6>{});
        item(c, u_tag, std::integral_constant<int, 7>{});
        item(c, u_tag, std::integral_constant<int, 8>{});
    };
    if (c_begin < c_end) {
        __syncthreads();                                               // styles are in LDS
        load_a(c_begin, std::integral_constant<int, 0>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        load_a(c_begin, std::integral_constant<int, 1>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 5>{});
        issue_b(c_begin, 0, std::integral_constant<int, 0>{});
        // pairs of chunks (LDS buffer and ring slots by chunk parity: compile time), then the odd one (an exit in the middle of
        // the pair spilled 62 registers)
        int cg = c_begin;
        for (; cg + 1 < c_end; cg += 2) {
            chunk(cg, std::integral_constant<int, 0>{});
            chunk(cg + 1, std::integral_constant<int, 1>{});
        }
        if (cg < c_end) chunk(cg, std::integral_constant<int, 0>{});
    }

    // ---- epilogue.  C/D layout of 16x16: column = lane & 15 (channel), row = 4 (lane >> 4) + r (position): the 4 registers of
    // tile (tm, tn) are columns n0 + 4g + r of patch row 4 wm + tm, channel co0 + 64 wn + 16 tn + i16.
    float* out = p.out + (size_t)ks * p.slab;
    float vmax = 0.f;
    const bool do_rgb = p.fused && p.rgb_part != nullptr;
    float rgbp[16 * 3];                                                // [position 4 tm + r][rgb]
#pragma unroll
    for (int i = 0; i < 16 * 3; ++i) rgbp[i] = 0.f;
    if constexpr (!LEGACY) {
        if (p.fused) {
            // The lane's operands in ONE batch (conv16_common.h): 16 noise values (row 4 wm + tm, column 4 g + r; rows and columns
            // past the image clamped) and, per N tile, dcoef, bias and the three rgb_w: 52 loads, one wait, in front of the first
            // store.  The arithmetic of an output and the order of the toRGB sums are the previous epilogue's: the same bits.
            const __amdgpu_buffer_rsrc_t r_nz = epi_rsrc(p.noise, (unsigned)(p.Ho * p.Wo) * 4u);
            const __amdgpu_buffer_rsrc_t r_d = epi_rsrc(p.dcoef ? p.dcoef + (size_t)b * p.Cout : nullptr, (unsigned)p.Cout * 4u);
            const __amdgpu_buffer_rsrc_t r_b = epi_rsrc(p.bias, (unsigned)p.Cout * 4u);
            const __amdgpu_buffer_rsrc_t r_w = epi_rsrc(do_rgb ? p.rgb_w + (size_t)b * 3 * p.Cout : nullptr, (unsigned)(3 * p.Cout) * 4u);
            const unsigned co_b = (unsigned)(co0 + wn * 64 + i16) * 4u;   // byte offset of the lane's channel in N tile 0; tile tn: + 64 tn
            float nz[16], dv[4], bv[4], rw3[4][3];
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    nz[tm * 4 + r] = epi_load(r_nz, (unsigned)(min(m0 + 4 * wm + tm, p.Ho - 1) * p.Wo + min(n0 + 4 * g + r, p.Wo - 1)) * 4u);
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) {
                dv[tn] = epi_load(r_d, co_b + 64u * tn);
                bv[tn] = epi_load(r_b, co_b + 64u * tn);
#pragma unroll
                for (int c = 0; c < 3; ++c) rw3[tn][c] = epi_load(r_w, (unsigned)(c * p.Cout) * 4u + co_b + 64u * tn);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) epi_landed(nz[i]);
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) {
                epi_landed(dv[tn]);
                epi_landed(bv[tn]);
#pragma unroll
                for (int c = 0; c < 3; ++c) epi_landed(rw3[tn][c]);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) nz[i] = p.noise ? nz[i] * p.noise_strength : 0.f;
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) dv[tn] = p.dcoef ? dv[tn] * sback : sback;      // (no bias, no toRGB: those loads returned 0)
            // the outputs, in place of their accumulators; an element outside the image counts for nothing in vmax (and its toRGB
            // sums belong to a position that is never written)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) {
                const bool row_ok = m0 + 4 * wm + tm < p.Ho;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = row_ok && n0 + 4 * g + r < p.Wo;
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn) {
                        const float v = lrelu_gain_clamp(acc[tm][tn][r] * dv[tn] + bv[tn] + nz[tm * 4 + r], p.act, p.alpha, p.gain, p.clamp);
                        acc[tm][tn][r] = v;
                        vmax = fmaxf(vmax, ok ? fabsf(v) : 0.f);
#pragma unroll
                        for (int c = 0; c < 3; ++c) rgbp[(tm * 4 + r) * 3 + c] = fmaf(v, rw3[tn][c], rgbp[(tm * 4 + r) * 3 + c]);
                    }
                }
            }
            // (in front of the stores: its look at the slot is a load, and the wait for it would wait for every store as well)
            if (p.y_absmax) publish_absmax(p.y_absmax, vmax, blockIdx.x * 4 + wave);
        } else {
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int tn = 0; tn < 4; ++tn)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[tm][tn][r] *= sback;       // (element by element: no packed fp32, build.sh)
        }
        // the stores, branch-free, through a resource over the rows of this tile that the image has (a row past the image is past
        // the resource); a column past the image gets EPI_OOB.  (No y wanted — the last layer in front of a fused toRGB: no stores.)
        if (p.out) {
            const unsigned row_b = (unsigned)(p.Wo * p.Cout) * 4u, col_b = (unsigned)p.Cout * 4u;
            const __amdgpu_buffer_rsrc_t r_y = epi_rsrc(out + ((size_t)b * p.Ho + m0) * p.Wo * p.Cout, (unsigned)min(8, p.Ho - m0) * row_b);
            const unsigned y_b = (unsigned)(4 * wm) * row_b + (unsigned)(n0 + 4 * g) * col_b + (unsigned)(co0 + wn * 64 + i16) * 4u;
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned off = n0 + 4 * g + r < p.Wo ? y_b + tm * row_b + r * col_b : EPI_OOB;
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn) epi_store(r_y, off + 64u * tn, acc[tm][tn][r]);
                }
        }
    }
    if constexpr (LEGACY) {
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        const int co = co0 + wn * 64 + tn * 16 + i16;
        float rw3[3] = {0.f, 0.f, 0.f};
        if (do_rgb) {
#pragma unroll
            for (int r = 0; r < 3; ++r) rw3[r] = p.rgb_w[((size_t)b * 3 + r) * p.Cout + co];
        }
        float d = sback, bs = 0.f;
        if (p.fused) {
            if (p.dcoef) d = p.dcoef[(size_t)b * p.Cout + co] * sback;
            if (p.bias) bs = p.bias[co];
        }
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) {
            const int m = m0 + 4 * wm + tm;
            if (m >= p.Ho) continue;
            float* rowp = out + ((size_t)b * p.Ho + m) * p.Wo * p.Cout + co;
            const float* nrow = (p.fused && p.noise) ? p.noise + (size_t)m * p.Wo : nullptr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 4 * g + r;
                const float nz = nrow ? nrow[min(n, p.Wo - 1)] * p.noise_strength : 0.f;
                if (n >= p.Wo) continue;
                float v = acc[tm][tn][r];
                if (p.fused) v = lrelu_gain_clamp(v * d + bs + nz, p.act, p.alpha, p.gain, p.clamp);
                else v *= sback;
                vmax = fmaxf(vmax, fabsf(v));
                if (p.out) rowp[n * p.Cout] = v;      // (NULL: only the fused toRGB sums are wanted)
#pragma unroll
                for (int c = 0; c < 3; ++c) rgbp[(tm * 4 + r) * 3 + c] = fmaf(v, rw3[c], rgbp[(tm * 4 + r) * 3 + c]);
            }
        }
    }
    if (p.fused && p.y_absmax) publish_absmax(p.y_absmax, vmax, blockIdx.x * 4 + wave);
    }   // LEGACY
    if (do_rgb) {
        // reduce-scatter over the 16 channel lanes (as in the 16-channel loop): afterwards lane i16 owns position i16 = 4 tm + r
        int n = 16 * 3;
#pragma unroll
        for (int mk = 8; mk >= 1; mk >>= 1) {
            n >>= 1;
            const bool up = (i16 & mk) != 0;
#pragma unroll
            for (int i = 0; i < 16 * 3 / 2; ++i) {
                if (i < n) {
                    const float keep = up ? rgbp[i + n] : rgbp[i];
                    const float give = up ? rgbp[i] : rgbp[i + n];
                    rgbp[i] = keep + __shfl_xor(give, mk);
                }
            }
        }
        const int m = m0 + 4 * wm + (i16 >> 2), nn = n0 + 4 * g + (i16 & 3);
        if (m < p.Ho && nn < p.Wo) {
            const int part = tn_blk * 2 + wn;
            float4* dst = reinterpret_cast<float4*>(p.rgb_part) + (((size_t)part * p.B + b) * p.Ho + m) * p.Wo + nn;
            *dst = make_float4(rgbp[0], rgbp[1], rgbp[2], 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The merged up-conv at F16X3 (KD = 4) on v_mfma_f32_16x16x32_f16 with 32-channel K chunks (upconv_bf16_kernel<4, 4, 0, LOOP>;
// launch_modconv_bf16 picks it where upconv_mfma16_takes).  What the 16-channel kernel above computes, issued the way of the
// 32-channel 3x3 loop:
//   * Same block tile (8 x 16 positions x 64 channels x four parity phases, 128 accumulator registers, two blocks per CU), same
//     stacked-row / fringe tiling, same grouping of the 9 (phase, tap) items by their four LDS shifts, same weight image, same A
//     parts (split4<4> of x . style . 2^-e), same split-K slices (cut in 32-channel chunks; an empty slice stores zeros).  A wave
//     owns patch rows 4 wm .. 4 wm + 3 (four 16-position M tiles) and channels 32 wn .. 32 wn + 31 (two 16-channel N tiles).
//   * 216 MFMAs per wave per barrier (9 items x 8 tiles x 3 products); the A fragments of a shift group are read once per chunk,
//     those of the next group per M tile under the last item of the current one.
//   * Weight fragments by buffer loads (SGPR resource, one per-lane offset for the kernel; tap / chunk / part in the scalar
//     offset, N tile in the immediate), ring of two items.
//   * Patch image per part [channel octet][position][16 B], 9 x 17 positions, octet stride 2560 B = 0 mod 256 B: every 16-lane
//     group of a ds_read_b128 reads 16 consecutive 16-B slots (one run per octet, the runs of a group's lanes 256 B apart modulo
//     256), every 16-lane group of a ds_write_b64 128 contiguous bytes.  ONE buffer resource covers the up_ns samples from b_lo on
//     (launch: that span stays below u16::OOB); slots outside an image — row m = H of the stacked pitch, columns outside 0 .. W-1,
//     rows past up_rows, the fringe tile's column -1 — carry the offset u16::OOB and load zeros.  The range-guard scale 2^-e of
//     each staged sample is folded into that sample's row of the style image in the prologue.
//   * The MFMA is issued with the weights as its first operand (16 output channels) and the activations as its second (16
//     positions) — the fragment layouts are the same, so are the products and their order: a lane's four accumulators are then
//     four consecutive channels of one position and y_t leaves as 16-byte stores (lane groups lane >> 4: 64 contiguous bytes per
//     position).  That is LOOP = 2.  LOOP = 1, the operands the other way round and 4-byte stores (16 channels x 4 positions per
//     instruction, four times the store instructions), was built and measured slower on every flagship layer (family sum 6027
//     against 5924 us, profiles/r08_upconv16_ab.log) and is not kept.
namespace u16 {
constexpr int CK = 32;                            // channels per K chunk
constexpr int LP = PW + 1, NPOS = (8 + 1) * LP;   // patch row pitch / positions (9 x 17)
constexpr int OCT = 2560;                         // bytes per channel octet of one part: NPOS x 16 B rounded up to 256 B
constexpr int A_PART = 4 * OCT, A_BUF = 2 * A_PART;
constexpr int A_PER_T = 5;                        // float4 slots per thread: 153 positions x 8 quads over 256 threads
constexpr unsigned OOB = 0xfffff000u;             // patch offset beyond every staged sample (+ the chunk offset: no 32-bit wrap)
static_assert(NPOS * 16 <= OCT && OCT % 256 == 0 && NPOS * 8 <= A_PER_T * 256 && 2 * A_BUF <= 48 * 1024, "patch layout");
constexpr size_t lds_bytes(int cin, int ns) { return (size_t)2 * A_BUF + (size_t)ns * (cin + 1) * sizeof(float); }
}  // namespace u16

template <int KD, int NW, int IO, int LOOP>
__global__ void __launch_bounds__(256, 2) upconv_bf16_kernel(const ConvParams p) {
    static_assert(KD == 4 && NW == 4 && IO == 0 && LOOP == 2, "the 32-channel loop is the 4-wave F16X3 up-conv");
    using namespace u16;
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    using namespace up_items;
    constexpr int RB = 2;                                              // weight ring slots
    constexpr int ST = 0;                                              // M tile after which an item converts its patch slot
    constexpr int S_SLOT[NITEM] = {-1, -1, 0, 1, -1, 2, 3, -1, 4};      // patch slot converted under each item
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    char* As = lds_raw;                                                // [2][2 parts][4 octets][OCT]
    float* Ss = reinterpret_cast<float*>(lds_raw + 2 * A_BUF);         // [up_ns][Cin] styles x 2^-e, then [up_ns] 2^e

    // ---- tiling: as in the 16-channel kernel
    unsigned id = p.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tiles_nu = p.Cout / 64;
    const int tn_blk = __builtin_amdgcn_readfirstlane(id % tiles_nu);  id /= tiles_nu;
    const int n_reg = p.up_tr * p.up_tw, n_tile = n_reg + p.up_nf;
    const int T = __builtin_amdgcn_readfirstlane(id % n_tile);         id /= n_tile;
    const int ks = __builtin_amdgcn_readfirstlane(id);
    const bool fringe = T >= n_reg;                                    // block-uniform
    const int RP = p.up_rp, R_total = p.up_rows;
    const int r0 = fringe ? (T - n_reg) * 64 : (T / p.up_tw) * 8, n0 = fringe ? 0 : (T % p.up_tw) * PW;
    const int co0 = tn_blk * 64;
    const int b_lo = min(max(r0 - 1, 0) / RP, p.B - 1);                // first sample the patch touches

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int g = lane >> 4, i16 = lane & 15;
    const int nch = p.Cin / CK;
    const int c_begin = __builtin_amdgcn_readfirstlane((int)(((long long)nch * ks) / p.ksplit));
    const int c_end = __builtin_amdgcn_readfirstlane((int)(((long long)nch * (ks + 1)) / p.ksplit));

    // styles of the up_ns samples from b_lo on (ones past the batch), each row times its sample's range-guard scale 2^-e
    float* Gb = Ss + p.up_ns * p.Cin;
    for (int sI = 0; sI < p.up_ns; ++sI) {
        const float* st = (p.styles && b_lo + sI < p.B) ? p.styles + (size_t)(b_lo + sI) * p.Cin : nullptr;
        float bk = 1.f;
        const float dn = style_range_guard(st, p.Cin, lane, &bk, p.x_absmax, p.w_absmax);
        for (int i = tid; i < p.Cin; i += 256) Ss[sI * p.Cin + i] = (st ? st[i] : 1.f) * dn;
        if (tid == 0) Gb[sI] = bk;
    }

    // ---- A staging: slot e = tid + 256 k holds channels 4q .. 4q+3 (q = 2 ((e >> 4) & 3) + (e & 1)) of patch position
    // 8 (e >> 6) + ((e >> 1) & 7); q does not depend on k.  Positions 153 .. 159 are the padding of the octet: zeros that nobody reads.
    const int nsamp = min(p.up_ns, p.B - b_lo);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x + (long long)b_lo * p.x_batch_stride), 0,
        (unsigned)(((long long)(nsamp - 1) * p.x_batch_stride + (long long)p.H * p.W * p.Cin) * 4), 0x00020000);
    const int qa = 2 * ((tid >> 4) & 3) + (tid & 1);
    // (registers that live through the K loop are scarce: slot k is 32 k positions after slot 0 in LDS, and the staged sample of
    // each slot, 0 .. 7, is three bits of the same register above the 14 bits of that address)
    static_assert(A_PART <= (1 << 14) && 14 + 3 * A_PER_T <= 32, "LDS address and sample indices share a register");
    unsigned aoff[A_PER_T];
    unsigned sels = (qa >> 1) * OCT + (8 * (tid >> 6) + ((tid >> 1) & 7)) * 16 + (qa & 1) * 8;
#pragma unroll
    for (int k = 0; k < A_PER_T; ++k) {
        const int pix = 8 * ((tid >> 6) + 4 * k) + ((tid >> 1) & 7);
        const int pi = pix / LP, pj = pix % LP;
        int r, n;
        if (!fringe) { r = r0 - 1 + pi; n = n0 - 1 + pj; }
        else { r = pj == 0 ? -1 : r0 + 8 * ((pj - 1) >> 1) + pi - 1; n = p.W - 1 + ((pj - 1) & 1); }
        const bool row_ok = r >= 0 && r < R_total;
        const int bb = row_ok ? r / RP : b_lo, m = r - bb * RP;
        const bool inside = pix < NPOS && row_ok && m < p.H && n >= 0 && n < p.W;
        const int sel = inside ? bb - b_lo : 0;
        aoff[k] = inside ? (unsigned)(((long long)sel * p.x_batch_stride + (long long)(m * p.W + n) * p.Cin + 4 * qa) * 4) : OOB;
        sels |= (unsigned)sel << (14 + 3 * k);
    }
    static_assert((8 * (3 + 4 * (A_PER_T - 1)) + 7) * 16 < OCT, "every slot lies inside its octet");
    // (in three parts of two, two and one slots: 8 staging registers instead of 20)
    float4 ra[2];
    auto load_a = [&](int chunk, auto part_tag) __attribute__((always_inline)) {
        constexpr int PT = decltype(part_tag)::value;
#pragma unroll
        for (int k = 0; k < (PT < 2 ? 2 : 1); ++k)
            ra[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, aoff[PT * 2 + k], chunk * CK * 4, 0));
    };
    auto store_a = [&](int chunk, auto buf_tag, auto k_tag) __attribute__((always_inline)) {
        constexpr int BUF = decltype(buf_tag)::value, k = decltype(k_tag)::value;
        const int sel = (int)((sels >> (14 + 3 * k)) & 7u);
        const float4 sv = *reinterpret_cast<const float4*>(Ss + chunk * CK + sel * p.Cin + 4 * qa);
        const int lds_a = (int)(sels & 0x3fffu) + k * 32 * 16;
        const float4 x = ra[k % 2];
        uint2 parts[2];
        split4<KD>(make_float4(x.x * sv.x, x.y * sv.y, x.z * sv.z, x.w * sv.w), parts);
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<uint2*>(As + BUF * A_BUF + q * A_PART + lds_a) = parts[q];
    };

    // ---- weight fragments: [part][tap][Cin/8][Cout][8] by buffer loads; lane offset (g Cout + co) x 16, N tile tn at +256 tn
    const int cq8 = p.Cin >> 3;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.wt), 0, (unsigned)(2 * 9 * cq8 * p.Cout) * 16u, 0x00020000);
    const unsigned boff = (unsigned)(g * p.Cout + co0 + wn * 32 + i16) * 16u;
    const int part_bytes = 9 * cq8 * p.Cout * 16, tap_bytes = cq8 * p.Cout * 16, chunk_bytes = 4 * p.Cout * 16;
    // activation fragment of M tile tm (patch row 4 wm + tm, column i16, + the group's shift), lane group g = channel octet g
    const char* const afrag = As + g * OCT + (4 * wm * LP + i16) * 16;

    f32x4v acc[4][4][2];                                               // phase, M tile, N tile
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) acc[f][tm][tn] = f32x4v{0.f, 0.f, 0.f, 0.f};

    constexpr PartOrder PO = kind_order(KD);
    u32x4 bq[RB][2][2];                                                // ring slot, N tile, part
    u32x4 af[4][2];                                                    // M tile, part (of the shift group being computed)
    auto issue_b = [&](int c, int w, auto slot_tag) __attribute__((always_inline)) {
        constexpr int SL = decltype(slot_tag)::value;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int so = q * part_bytes + w * tap_bytes + c * chunk_bytes;   // scalar
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) bq[SL][tn][q] = __builtin_amdgcn_raw_buffer_load_b128(rw, boff + 256 * tn, so, 0);
        }
    };
    auto read_a = [&](auto u_tag, auto g_tag, auto tm_tag) __attribute__((always_inline)) {
        constexpr int UU = decltype(u_tag)::value, G = decltype(g_tag)::value, TMI = decltype(tm_tag)::value;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            af[TMI][q] = *reinterpret_cast<const u32x4*>(afrag + UU * A_BUF + q * A_PART + (TMI * LP + group_pos(G, LP)) * 16);
    };
    // item = (phase, tap) I of chunk c: the weights of item I + RB - 1 into the ring, then per M tile its 6 MFMAs followed, under the
    // last item of a shift group, by the reads of that tile's fragments for the next group; the patch of chunk c+1 is fetched at
    // three parts (at items 0, 3 and 6) and converted one slot per item into the other LDS buffer under items 2, 3 | 5, 6 | 8
    auto item = [&](int c, auto u_tag, auto i_tag) __attribute__((always_inline)) {
        constexpr int UU = decltype(u_tag)::value, I = decltype(i_tag)::value, G = I_GRP[I], F = I_PHASE[I];
        constexpr int SL = (UU * NITEM + I) % RB, IN = I + RB - 1;
        issue_b(c + IN / NITEM, I_W[IN % NITEM], std::integral_constant<int, (SL + RB - 1) % RB>{});
        if constexpr (I == 0) load_a(min(c + 1, c_end - 1), std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        auto tile = [&](auto tm_tag) __attribute__((always_inline)) {
            constexpr int TMI = decltype(tm_tag)::value;
#pragma unroll
            for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    const f16x8 xa = __builtin_bit_cast(f16x8, af[TMI][PO.pa[pr]]), wb = __builtin_bit_cast(f16x8, bq[SL][tn][PO.pb[pr]]);
                    acc[F][TMI][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb, xa, acc[F][TMI][tn], 0, 0, 0);
                }
            if constexpr (I + 1 < NITEM && I_GRP[(I + 1) % NITEM] != G) read_a(u_tag, std::integral_constant<int, G + 1>{}, tm_tag);
            if constexpr (TMI == ST && S_SLOT[I] >= 0)
                store_a(min(c + 1, c_end - 1), std::integral_constant<int, 1 - UU>{}, std::integral_constant<int, (S_SLOT[I] < 0 ? 0 : S_SLOT[I])>{});
            if constexpr (TMI == ST && (I == 3 || I == 6))
                load_a(min(c + 1, c_end - 1), std::integral_constant<int, I / 3>{});
            __builtin_amdgcn_sched_barrier(0);
        };
        tile(std::integral_constant<int, 0>{});
        tile(std::integral_constant<int, 1>{});
        tile(std::integral_constant<int, 2>{});
        tile(std::integral_constant<int, 3>{});
    };
    auto chunk = [&](int c, auto u_tag) __attribute__((always_inline)) {
        __syncthreads();                                               // publishes the patch of chunk c
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        read_a(u_tag, std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
        __builtin_amdgcn_sched_barrier(0);
        item(c, u_tag, std::integral_constant<int, 0>{});
        item(c, u_tag, std::integral_constant<int, 1>{});
        item(c, u_tag, std::integral_constant<int, 2>{});
        item(c, u_tag, std::integral_constant<int, 3>{});
        item(c, u_tag, std::integral_constant<int, 4>{});
        item(c, u_tag, std::integral_constant<int, 5>{});
        item(c, u_tag, std::integral_constant<int, 6>{});
        item(c, u_tag, std::integral_constant<int, 7>{});
        item(c, u_tag, std::integral_constant<int, 8>{});
    };
    static_assert((2 * NITEM) % RB == 0, "ring slots must repeat every chunk pair");
    __syncthreads();                                                   // styles and back-scales are in LDS
    if (c_begin < c_end) {
        load_a(c_begin, std::integral_constant<int, 0>{});
        issue_b(c_begin, I_W[0], std::integral_constant<int, 0>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        load_a(c_begin, std::integral_constant<int, 1>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
        load_a(c_begin, std::integral_constant<int, 2>{});
        store_a(c_begin, std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
        // pairs of chunks (LDS buffer and ring slots by chunk parity: compile time), then the odd one
        int cg = c_begin;
        for (; cg + 1 < c_end; cg += 2) {
            chunk(cg, std::integral_constant<int, 0>{});
            chunk(cg + 1, std::integral_constant<int, 1>{});
        }
        if (cg < c_end) chunk(cg, std::integral_constant<int, 0>{});
    }

    // ---- raw stores of the four phases: y_t[2m + (f>>1)][2n + (f&1)], extents (H+1-(f>>1)) x (W+1-(f&1)), times the sample's 2^e.
    // C/D layout of 16x16: column = lane & 15 = tile column of patch row 4 wm + tm, rows 4 (lane >> 4) + v = channels 4g .. 4g+3
    // of the N tile (one 16-byte store).
    // (the lane index from the execution mask, counted up from a zero the compiler cannot see before the loop: no register holds a
    // thread index through the K loop for the stores)
    unsigned zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
    const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero)), ge = lane_e >> 4, ie = lane_e & 15;
    float* out = p.out + (size_t)ks * p.slab;
    auto put = [&](auto f_tag, auto tm_tag, size_t pos, float sb) __attribute__((always_inline)) {
        constexpr int F = decltype(f_tag)::value, TMI = decltype(tm_tag)::value;
        float* dst = out + pos * p.Cout + co0 + wn * 32;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            // (component by component: a vector multiply would be packed fp32 arithmetic, which build.sh keeps out of the library)
            const f32x4v a = acc[F][TMI][tn];
            *reinterpret_cast<f32x4v*>(dst + 16 * tn + 4 * ge) = f32x4v{a[0] * sb, a[1] * sb, a[2] * sb, a[3] * sb};
        }
    };
    auto rows = [&](auto tm_tag) __attribute__((always_inline)) {
        constexpr int TMI = decltype(tm_tag)::value;
        const int ru = r0 + 4 * wm + TMI, bu = ru / RP;
        {
            const int j = ie;                                          // tile column
            // regular tile: stacked row r0 + patch row, image column n0 + j; fringe tile: tile column j is image column W of
            // row block j >> 1 for odd j (even j: column W-1, which the regular tiles own), even-column parities only
            int r = ru, bb = bu;                                        // (block-uniform branch: the regular tiles divide on the scalar ALU)
            if (fringe) { r += 8 * (j >> 1); bb = r / RP; }
            const int n = fringe ? p.W : n0 + j, m = r - bb * RP;
            if (r >= R_total || (fringe && !(j & 1))) return;
            const float sb = Gb[min(max(bb - b_lo, 0), p.up_ns - 1)];
            auto phase = [&](auto f_tag) __attribute__((always_inline)) {
                constexpr int F = decltype(f_tag)::value, FY = F >> 1, FX = F & 1;
                if (m >= p.H + 1 - FY || n >= p.W + 1 - FX) return;
                put(f_tag, tm_tag, ((size_t)bb * p.Ho + 2 * m + FY) * p.Wo + 2 * n + FX, sb);
            };
            phase(std::integral_constant<int, 0>{});
            phase(std::integral_constant<int, 1>{});
            phase(std::integral_constant<int, 2>{});
            phase(std::integral_constant<int, 3>{});
        }
    };
    rows(std::integral_constant<int, 0>{});
    rows(std::integral_constant<int, 1>{});
    rows(std::integral_constant<int, 2>{});
    rows(std::integral_constant<int, 3>{});
}

template <int NP, int TM>
static size_t bf16_lds_bytes(int cin) {
    constexpr int PH = 2 * TM * 32 / PW;
    return (size_t)2 * NP * (PH + 2) * RowPitch<NP>::value * APITCH + (size_t)(cin + 8) * sizeof(float);   // + guard scratch
}

template <int KD>
static void launch_group(const Plan& pl, int phase0, int nphase, int ntaps, int cin, bool epi_legacy, hipStream_t s) {
    const dim3 grid(pl.grid.x, (unsigned)nphase, 1);
    const size_t lds = bf16_lds_bytes<kind_parts_a(KD), 2>(cin);
    if constexpr (KD == 4) {            // developer A/B of the epilogue (modconv_plan.h)
        if (ntaps == 9 && epi_legacy) {
            modconv_bf16_kernel<4, 2, 9, 4><<<grid, 256, lds, s>>>(pl.p, phase0);
            return;
        }
    }
    switch (ntaps) {
        case 9: modconv_bf16_kernel<KD, 2, 9><<<grid, 256, lds, s>>>(pl.p, phase0); break;
        case 4: modconv_bf16_kernel<KD, 2, 4><<<grid, 256, lds, s>>>(pl.p, phase0); break;
        case 2: modconv_bf16_kernel<KD, 2, 2><<<grid, 256, lds, s>>>(pl.p, phase0); break;
        default: modconv_bf16_kernel<KD, 2, 1><<<grid, 256, lds, s>>>(pl.p, phase0); break;
    }
}

// mode CONVS2_BWD, the four parity phases merged in one block (make_plan: merged_s2; grid.y = 1)
template <int KD>
static void launch_s2_merged(const Plan& pl, int cin, hipStream_t s) {
    modconv_bf16_kernel<KD, 2, 0><<<pl.grid, 256, bf16_lds_bytes<kind_parts_a(KD), 2>(cin), s>>>(pl.p, 0);
}

// LDS of the merged up-conv: the two patch buffers + styles and range-guard scales of up_ns samples; beyond the 64 KB default the
// kernel's dynamic-LDS limit is raised once per instantiation
// Raise a kernel's dynamic-LDS limit beyond the 64 KB default.  The attribute belongs to the device that is current when it is set,
// so it is set once per (kernel, device): `raised` (one per kernel) keeps a bit per device ordinal.
static int raise_dynamic_lds(const void* fn, int bytes, std::atomic<unsigned long long>& raised, const char* what) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    HFAGP_REQUIRE(e == hipSuccess && dev >= 0 && dev < 64, HFAGP_ELAUNCH, "%s: hipGetDevice: %s", what, hipGetErrorString(e));
    const unsigned long long bit = 1ull << dev;
    if (raised.load(std::memory_order_acquire) & bit) return HFAGP_OK;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    HFAGP_REQUIRE(e == hipSuccess, HFAGP_ELAUNCH, "%s: cannot raise dynamic LDS to %d bytes on device %d: %s", what, bytes, dev,
                  hipGetErrorString(e));
    raised.fetch_or(bit, std::memory_order_release);
    return HFAGP_OK;
}

template <int KD, int NW, int IO>
static int launch_up_one(const Plan& pl, int cin, hipStream_t s) {
    const size_t lds = bf16_lds_bytes<kind_parts_a(KD), 2>(0) + (size_t)(pl.p.up_ns * (cin + 2)) * sizeof(float);
    static std::atomic<unsigned long long> raised{0};
    if (lds > 64 * 1024) {
        const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&upconv_bf16_kernel<KD, NW, IO>), 128 * 1024, raised,
                                         "upconv_bf16_kernel");
        if (rc != HFAGP_OK) return rc;
    }
    upconv_bf16_kernel<KD, NW, IO><<<pl.grid, NW * 64, lds, s>>>(pl.p);
    return HFAGP_OK;
}

// the 32-channel loop of the F16X3 up-conv (upconv_mfma16_takes)
static int launch_up16(const Plan& pl, int cin, hipStream_t s) {
    // (make_plan stages at most 8 samples and Cin <= 512: 57,376 B at the most, under the 64 KB a kernel gets without asking and
    // two blocks per CU; the 16-channel loop above is the one that has to raise its limit)
    static_assert(u16::lds_bytes(512, 8) <= 64 * 1024, "the 32-channel up-conv loop stays within the default dynamic LDS");
    HFAGP_REQUIRE(cin <= 512 && pl.p.up_ns <= 8, HFAGP_EUNSUPPORTED, "modconv (merged up-conv, 32-channel loop): Cin=%d up_ns=%d",
                  cin, pl.p.up_ns);
    const size_t lds = u16::lds_bytes(cin, pl.p.up_ns);
    upconv_bf16_kernel<4, 4, 0, 2><<<pl.grid, 256, lds, s>>>(pl.p);
    return HFAGP_OK;
}

// fp16-storage variants (KD = 1 only): io = x_f16 | y_f16 << 1
static int launch_up_io(const Plan& pl, int cin, int io, hipStream_t s) {
    const bool w8 = pl.up_waves == 8;
    if (io == 2) return w8 ? launch_up_one<1, 8, 2>(pl, cin, s) : launch_up_one<1, 4, 2>(pl, cin, s);
    return w8 ? launch_up_one<1, 8, 3>(pl, cin, s) : launch_up_one<1, 4, 3>(pl, cin, s);
}

template <int KD>
static int launch_up(const Plan& pl, int cin, hipStream_t s) {
    if constexpr (KD != 3) {            // (three parts: the 8-wave variant would spill; make_plan never asks for it)
        if (pl.up_waves == 8) return launch_up_one<KD, 8, 0>(pl, cin, s);
    }
    return launch_up_one<KD, 4, 0>(pl, cin, s);
}

// f(std::integral_constant<int, KD>{}) for the operand kind kd (kind_of(precision), not 0) as a compile-time constant
template <class F>
static auto with_kind(int kd, F&& f) {
    switch (kd) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 5: return f(std::integral_constant<int, 5>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

int launch_modconv_bf16(const HfagpModconvArgs* a, Plan& pl, hipStream_t s) {
    // (the 4-wave block of the merged up-conv, both loops, tiles Cout in 64s; fp16 storage asks for 128 below)
    HFAGP_REQUIRE(a->Cin % CKB == 0 && (a->Cout % BNB == 0 || (a->Cout % BNB >= 96 && !pl.merged_up) ||
                                        (pl.merged_up && pl.up_waves == 4 && a->Cout % 64 == 0)), HFAGP_EUNSUPPORTED,
                  "modconv (16-bit MFMA): Cin=%d must be a multiple of %d and Cout=%d of %d (or 96 mod 128, 512-B tail pad; the merged "
                  "up-conv: of 64)", a->Cin, CKB, a->Cout, BNB);
    HFAGP_REQUIRE(pl.bn == BNB && pl.bm == 128, HFAGP_EUNSUPPORTED, "modconv (16-bit MFMA): unexpected plan");
    HFAGP_REQUIRE(a->Cin <= 512, HFAGP_EUNSUPPORTED, "modconv (16-bit MFMA): Cin=%d > 512 (style image in LDS)", a->Cin);
    // (modconv_bf16_kernel's epilogues store through a buffer resource over the up to 16 output rows of a tile: 32-bit byte offsets
    // below EPI_OOB; the merged up-conv kernels address y_t with pointers)
    HFAGP_REQUIRE(pl.merged_up || (long long)pl.p.Wo * pl.p.Cout < (1ll << 25), HFAGP_EUNSUPPORTED,
                  "modconv (16-bit MFMA): an output row of %d x %d elements exceeds the 32-bit tile offsets", pl.p.Wo, pl.p.Cout);
    const int kd = kind_of(a->precision);
    HFAGP_REQUIRE(kd != 0, HFAGP_EBADARG, "modconv: unknown precision %d", a->precision);
    const int io = (a->x_f16 ? 1 : 0) | (a->y_f16 ? 2 : 0);
    if (io) {
        const ConvParams& q = pl.p;
        HFAGP_REQUIRE(kd == 1 && q.ksplit * q.nslab == 1 && a->Cout % BNB == 0 &&
                          ((a->mode == HFAGP_CONV3X3 && io == 3) || (a->mode == HFAGP_CONVT3X3_UP2 && (io & 2))),
                      HFAGP_EUNSUPPORTED, "modconv: fp16 storage needs precision F16, no split-K, Cout %% 128 == 0 and mode 0 "
                                          "(x and y fp16) or mode 1 (y fp16); got precision %d mode %d x_f16 %d y_f16 %d ksplit %d",
                      a->precision, a->mode, a->x_f16, a->y_f16, q.ksplit);
        if (a->mode == HFAGP_CONVT3X3_UP2) {
            // (make_plan merges EVERY 16-bit up-conv, at any grid and batch: this cannot fire; Cin <= 512 is checked above)
            HFAGP_REQUIRE(pl.merged_up, HFAGP_EUNSUPPORTED, "modconv: fp16 storage of the up-conv needs the merged four-phase "
                                                            "kernel (every 16-bit up-conv plan)");
            HFAGP_REQUIRE(q.up_ns <= 1 || (long long)q.up_ns * a->x_batch_stride * (a->x_f16 ? 2 : 4) < (1ll << 32), HFAGP_EUNSUPPORTED,
                          "modconv (merged up-conv): %d samples of %lld elements exceed the 32-bit patch offsets", q.up_ns,
                          (long long)a->x_batch_stride);
            const int rc = launch_up_io(pl, a->Cin, io, s);
            if (rc != HFAGP_OK) return rc;
            return check_launch("modconv_fwd (fp16 storage, merged up-conv)");
        }
        const dim3 grid(pl.grid.x, 1, 1);
        modconv_bf16_kernel<1, 2, 9, 3><<<grid, 256, bf16_lds_bytes<1, 2>(a->Cin), s>>>(pl.p, 0);
        return check_launch("modconv_fwd (fp16 storage)");
    }
    // the kernel is specialised on the tap count: one launch per run of phases with the same number of taps
    // (3x3: one; stride-2 transposed conv and its adjoint: 4 | 2, 2 | 1)
    const ConvParams& p = pl.p;
    if (pl.merged_up) {                 // one block for the four phases (grid.y = 1)
        // (a block addresses the up_ns samples its tile can touch with 32-bit byte offsets from the first one)
        HFAGP_REQUIRE(p.up_ns <= 1 || (long long)p.up_ns * a->x_batch_stride * (a->x_f16 ? 2 : 4) < (1ll << 32), HFAGP_EUNSUPPORTED,
                      "modconv (merged up-conv): %d samples of %lld elements exceed the 32-bit patch offsets", p.up_ns,
                      (long long)a->x_batch_stride);
        // (the 32-channel loop marks a patch slot outside the images by the offset u16::OOB: the staged span must end below it)
        const bool loop32 = pl.up_waves == 4 && upconv_mfma16_takes(a) &&
                            (long long)p.up_ns * a->x_batch_stride * 4 <= (long long)u16::OOB;
        const int rc = loop32 ? launch_up16(pl, a->Cin, s)
                              : with_kind(kd, [&](auto k) { return launch_up<decltype(k)::value>(pl, a->Cin, s); });
        if (rc != HFAGP_OK) return rc;
        return check_launch("modconv_fwd (16-bit MFMA, merged up-conv)");
    }
    if (pl.merged_s2) {
        with_kind(kd, [&](auto k) { launch_s2_merged<decltype(k)::value>(pl, a->Cin, s); });
        return check_launch("modconv_fwd (16-bit MFMA, merged adjoint of the up-conv)");
    }
    if (conv9_mfma16_takes(a)) {        // the forward 3x3 conv at F16X3: the 32-channel 16x16x32 loop
        if (conv_epilogue_legacy()) modconv_bf16_kernel<4, 2, 9, 0, 3><<<pl.grid, 256, c9::lds_bytes(a->Cin), s>>>(p, 0);
        else modconv_bf16_kernel<4, 2, 9, 0, 1><<<pl.grid, 256, c9::lds_bytes(a->Cin), s>>>(p, 0);
        return check_launch("modconv_fwd (16-bit MFMA, 32-channel loop)");
    }
    for (int p0 = 0; p0 < p.nphase;) {
        int n = 1;
        while (p0 + n < p.nphase && p.phase[p0 + n].ntaps == p.phase[p0].ntaps) ++n;
        const int nt = p.phase[p0].ntaps;
        HFAGP_REQUIRE(nt == 9 || nt == 4 || nt == 2 || nt == 1, HFAGP_EUNSUPPORTED, "modconv (16-bit MFMA): %d taps", nt);
        const bool epi_legacy = a->mode == HFAGP_CONV3X3 && conv_epilogue_legacy();
        with_kind(kd, [&](auto k) { launch_group<decltype(k)::value>(pl, p0, n, nt, a->Cin, epi_legacy, s); });
        p0 += n;
    }
    return check_launch("modconv_fwd (16-bit MFMA)");
}

}  // namespace hfagp
