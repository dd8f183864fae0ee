// Porous zones on the device, beside the momentum assembly sweeps (fv_kernels.hip, ldu_kernels.hip), which add the coefficient themselves (porous.hpp: porous_diag):
//   k_porous_force     on request: per zone S V, S a V and F_q = S a V C_q(U) U_q over the zones' cells only, from a compact cell list.  One lane per list entry,
//                      256-lane blocks, no atomics: a block serves one zone and leaves one partial per sum (block_reduce_store); the shared fold
//                      (launch_reduce_finalize) adds the partials in a fixed order, so the sums have the same bits from run to run
//   k_porous_zone_f64  the read-out "porousZone": the cell-to-zone bytes as doubles
// Every bracket is one IEEE operation (-ffp-contract=off).  Geometry-free: compiled once, for the block and the general-mesh solver alike.
#include "device_util.hpp"
#include "fv_linalg_kernels.hpp"
#include "porous.hpp"

namespace fy {
namespace {

__global__ __launch_bounds__(256) void k_porous_force(int n_padded, const int32_t* __restrict__ cells, const int32_t* __restrict__ blk_zone, const double* __restrict__ vol,
                                                      const PorousDev* __restrict__ por, double nu, const double* __restrict__ U, const double* __restrict__ alpha,
                                                      double* __restrict__ partials) {
    const int z = blk_zone[blockIdx.x];                 // uniform over the block: the barrier inside block_reduce_store is reached by all lanes or by none
    if (z < 0) return;
    double v[kPorousSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int c = e < n_padded ? cells[e] : -1;
    if (c >= 0) {
        const double V = vol[e], aV = alpha ? alpha[c] * V : V;
        const double u0 = U[3 * (size_t)c], u1 = U[3 * (size_t)c + 1], u2 = U[3 * (size_t)c + 2];
        double pc[3];
        porous_diag(por, z, nu, aV, u0, u1, u2, pc);
        v[0] = V; v[1] = aV; v[2] = pc[0] * u0; v[3] = pc[1] * u1; v[4] = pc[2] * u2;
    }
    const int mx[kPorousSums] = {0, 0, 0, 0, 0};
    block_reduce_store<kPorousSums>(v, mx, partials + (size_t)z * kPorousSums * gridDim.x, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(256) void k_porous_zone_f64(int n, const unsigned char* __restrict__ zone_of, double* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n) out[c] = (double)zone_of[c];
}

}  // namespace

int launch_porous_force(hipStream_t s, int n_padded, const int32_t* cells, const int32_t* blk_zone, const double* vol, const PorousDev* por, double nu, const double* U,
                        const double* alpha, double* partials) {
    hipLaunchKernelGGL(k_porous_force, dim3(red_blocks(n_padded)), dim3(256), 0, s, n_padded, cells, blk_zone, vol, por, nu, U, alpha, partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}
int launch_porous_zone_f64(hipStream_t s, int n, const unsigned char* zone_of, double* out) {
    return launch_n(s, k_porous_zone_f64, n, 256, n, zone_of, out);
}

}  // namespace fy
