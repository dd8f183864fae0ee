// Open boundaries on the general mesh (open_boundary.hpp): the inflow mask of the boundary faces and its three sums.  One lane per boundary face, 256-lane blocks,
// no atomics: the lane stores its own byte, the block leaves one partial per sum (block_reduce_store), the shared fold adds the partials in a fixed order.
#include <algorithm>

#include "device_util.hpp"
#include "fv_linalg_kernels.hpp"
#include "open_boundary.hpp"

namespace fy {
namespace {

// the grid is red_blocks(nb) blocks (what the fold expects): the blocks past the last face store zeros.  One lane per face, no grid-stride loop: the launcher relies
// on red_blocks(n) >= ceil(n / 256) (fv_linalg_kernels.hpp: the block count rounded UP to a multiple of 8, never capped) and checks it
__global__ __launch_bounds__(256) void k_ldu_open_faces(LduGeo g, const int32_t* __restrict__ open_patch, const double* __restrict__ phi, uint8_t* __restrict__ mask,
                                                        double* __restrict__ partials) {
    double v[OPEN_SUMS] = {0.0, 0.0, 0.0};
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < g.nFaces - g.nInt) {
        uint8_t in = 0;
        if (open_patch[g.patch_of[b]]) {
            const double fl = phi[g.nInt + b];
            in = fl < 0.0 ? 1 : 0;
            v[OPEN_INFLOW_FACES] = in ? 1.0 : 0.0;
            v[OPEN_INFLOW_FLUX] = in ? fl : 0.0;
            v[OPEN_OUTFLOW_FLUX] = in ? 0.0 : fl;
        }
        mask[b] = in;
    }
    const int mx[OPEN_SUMS] = {0, 0, 0};
    block_reduce_store<OPEN_SUMS>(v, mx, partials, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(256) void k_ldu_open_mask_f64(int nb, const uint8_t* __restrict__ mask, double* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb) out[b] = mask[b] ? 1.0 : 0.0;
}

}  // namespace

int launch_ldu_open_faces(hipStream_t s, LduGeo g, const int32_t* open_patch, const double* phi, uint8_t* mask, double* partials) {
    const int nb = g.nFaces - g.nInt;
    if ((size_t)red_blocks(nb) * 256 < (size_t)nb) return fail(FY_ERR_INVALID, "launch_ldu_open_faces: %d blocks do not cover %d boundary faces", red_blocks(nb), nb);
    hipLaunchKernelGGL(k_ldu_open_faces, dim3(red_blocks(nb)), dim3(256), 0, s, g, open_patch, phi, mask, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}
int launch_ldu_open_mask_f64(hipStream_t s, int nb, const uint8_t* mask, double* out) {
    if (nb <= 0) return FY_OK;
    hipLaunchKernelGGL(k_ldu_open_mask_f64, dim3(div_up((size_t)nb, 256)), dim3(256), 0, s, nb, mask, out);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

}  // namespace fy
