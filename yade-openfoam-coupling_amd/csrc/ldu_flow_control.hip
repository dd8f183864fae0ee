// Flow-rate control on the general mesh (fy_flow_control_desc; DESIGN.md section 3 "Flow-rate control"): the role of OpenFOAM's meanVelocityForce fvOption
// [OF-6 meanVelocityForce.C, as recalled].  Three kernels, one lane per cell (or per component of a cell), 256-lane blocks, no atomics:
//   k_ldu_flow_source  per momentum assembly: gradP0 += dGradP, dGradP = 0 on the device, and the effective external source x + flowDir gradP0
//   k_ldu_flow_sums    per corrector: the block partials of S (flowDir . U) w V and S rAU w V (folded by launch_reduce_finalize, fixed order)
//   k_ldu_flow_apply   per corrector: dGradP from the two folded sums in every lane's prologue, then U += flowDir (rAU dGradP)
// Every bracket is one IEEE operation (-ffp-contract=off).  The state lives in two records that trade places at each assembly (LduFlow::cur is the one the step
// reads; the host flips it without knowing a value): k_ldu_flow_source reads one and writes the other, so no lane can see a half-updated record.
#include <algorithm>

#include "device_util.hpp"
#include "ldu.hpp"

namespace fy {
namespace {

// one thread per component of a cell.  Every lane forms the new gradP0 from the record of the last assembly; lane 0 of block 0 files it in the other record
__global__ __launch_bounds__(256) void k_ldu_flow_source(size_t n3, const double* __restrict__ st_in, double* __restrict__ st_out, const double* __restrict__ ext,
                                                         double dx, double dy, double dz, int increment, double* __restrict__ out) {
    const double dG = st_in[FLOW_DGRADP];
    const double g0 = st_in[FLOW_GRADP0] + dG;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) { st_out[FLOW_GRADP0] = g0; st_out[FLOW_DGRADP] = 0.0; st_out[FLOW_UBAR] = st_in[FLOW_UBAR]; st_out[FLOW_RAUAVE] = st_in[FLOW_RAUAVE]; }
    if (e >= n3) return;
    const int q = (int)(e % 3);
    const double d = q == 0 ? dx : q == 1 ? dy : dz;
    // increment (a later PIMPLE outer iteration): `out` is the momentum source that already holds flowDir times the gradP0 of the assembly before; it gains the difference
    if (increment) out[e] = out[e] + d * dG;
    else out[e] = (ext ? ext[e] : 0.0) + d * g0;
}

// slot 0 = S (flowDir . U_c) w_c V_c, slot 1 = S rAU_c w_c V_c; w = alpha, or 1 (alpha null).  Lanes past the last cell (and the padding blocks) hold 0
__global__ __launch_bounds__(256) void k_ldu_flow_sums(int n, const double* __restrict__ U, const double* __restrict__ rAU, const double* __restrict__ V,
                                                       const double* __restrict__ alpha, double dx, double dy, double dz, double* __restrict__ partials) {
    double v[2] = {0.0, 0.0};
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n) {
        const double dot = (dx * U[3 * (size_t)c] + dy * U[3 * (size_t)c + 1]) + dz * U[3 * (size_t)c + 2];
        const double vol = V[c];
        if (alpha) { const double w = alpha[c]; v[0] = (dot * w) * vol; v[1] = (rAU[c] * w) * vol; }
        else { v[0] = dot * vol; v[1] = rAU[c] * vol; }
    }
    const int mx[2] = {0, 0};
    block_reduce_store<2>(v, mx, partials, (int)blockIdx.x, (int)gridDim.x);
}

// the launch-boundary reduce: every lane reads the two folded sums and forms dGradP itself; lane 0 of block 0 files the record and counts the correction
__global__ __launch_bounds__(256) void k_ldu_flow_apply(int n, const double* __restrict__ sums, double* __restrict__ st, unsigned long long* __restrict__ count,
                                                        double mag_ubar, double relax, double total_volume, double dx, double dy, double dz,
                                                        const double* __restrict__ rAU, double* __restrict__ U) {
    const double ubar = sums[0] / total_volume;
    const double rAUave = sums[1] / total_volume;
    const double dG = (relax * (mag_ubar - ubar)) / rAUave;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c == 0) { st[FLOW_DGRADP] = dG; st[FLOW_UBAR] = ubar; st[FLOW_RAUAVE] = rAUave; *count += 1ull; }
    if (c >= n) return;
    const double a = rAU[c] * dG;
    double* u = U + 3 * (size_t)c;
    u[0] = u[0] + dx * a;
    u[1] = u[1] + dy * a;
    u[2] = u[2] + dz * a;
}

}  // namespace

int launch_ldu_flow_source(hipStream_t s, int n_cells, const double* st_in, double* st_out, const double* ext, const double* dir, bool increment, double* out) {
    const size_t n3 = 3 * (size_t)n_cells;
    hipLaunchKernelGGL(k_ldu_flow_source, dim3(std::max(1u, div_up(n3, 256))), dim3(256), 0, s, n3, st_in, st_out, ext, dir[0], dir[1], dir[2], increment ? 1 : 0, out);
    FY_LAUNCH_CHECK();
    return FY_OK;
}
int launch_ldu_flow_sums(hipStream_t s, int n_cells, const double* U, const double* rAU, const double* V, const double* alpha, const double* dir, double* partials) {
    hipLaunchKernelGGL(k_ldu_flow_sums, dim3(ldu_red_blocks(n_cells)), dim3(256), 0, s, n_cells, U, rAU, V, alpha, dir[0], dir[1], dir[2], partials);
    FY_LAUNCH_CHECK();
    return FY_OK;
}
int launch_ldu_flow_apply(hipStream_t s, int n_cells, const double* sums, double* st, unsigned long long* count, double mag_ubar, double relax, double total_volume,
                          const double* dir, const double* rAU, double* U) {
    hipLaunchKernelGGL(k_ldu_flow_apply, dim3(std::max(1u, div_up((size_t)n_cells, 256))), dim3(256), 0, s, n_cells, sums, st, count, mag_ubar, relax, total_volume,
                       dir[0], dir[1], dir[2], rAU, U);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

}  // namespace fy
