// Surface normals along ray lists (hfagp.h hfagp_raymarch_rays_normals / _normals_bwd / _normals_bwd_rays): the list instantiations
// of the three normals kernels — raymarch_normals_kernel<.., LIST = true> (raymarch_normals.hip),
// raymarch_normals_bwd_kernel<.., LIST = true> (raymarch_normals_bwd.hip), raymarch_normals_camera_rays_kernel
// (raymarch_normals_camera.hip) — and their entry points, as a unit of their own.  The kernels, their launchers and the entry points
// are written next to the grid's in those three sources, which differ from the list forms under `if constexpr (LIST)` alone; with
// HFAGP_RAY_LIST_UNIT defined each of them leaves out its grid entry point and emits the list's instead, so that the grid units
// hold the grid kernels and nothing else, as they did.  (build.sh hashes the three sources into this unit's object.)
#define HFAGP_RAY_LIST_UNIT
#include "raymarch_normals.hip"
#include "raymarch_normals_bwd.hip"
#include "raymarch_normals_camera.hip"
