/* mvs_region_launch.h -- launch geometry of the eval path's region kernels in libmvs_cost_volume.so: host-only
 * arithmetic over the arguments of a launch, for tests and tools (csrc/region_conv.h holds the helpers the
 * launchers themselves use).
 *
 * Additive: mvs_abi_version() is unchanged.  Status codes are those of mvs_cost_volume.h; nothing here touches a
 * device.
 */
#ifndef MVS_REGION_LAUNCH_H
#define MVS_REGION_LAUNCH_H

#include "../mvs_cost_volume.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The stride-2 cell kernel's launch (csrc/conv3d_region.hip, conv3d_s2_cells_kernel) for an output region of
 * out_size[3] voxels (z, y, x): geometry[6] = { cell extent in z, cell extent in y, 16-row blocks per wave,
 * GEMM rows (cells x out_size[2]), waves, workgroups per sample (a multiple of 8) }.
 * Returns 1 when mvs_conv3d_region_fwd(MVS_CONV_S2) runs that kernel for (c_in, c_out) -- from the fp32 volume,
 * NCDHW or channel quads, without y_bound and without MVS_CONV_PER_LANE -- and 0 when it runs the per-lane kernel
 * (the geometry is filled in either way); MVS_ERR_INVALID_ARGUMENT for a null pointer or a size <= 0,
 * MVS_ERR_TOO_LARGE for 2^31 output voxels and more. */
int mvs_conv3d_s2_cells_geometry(int c_in, int c_out, const int* out_size, long long* geometry);

#ifdef __cplusplus
}
#endif

#endif /* MVS_REGION_LAUNCH_H */
