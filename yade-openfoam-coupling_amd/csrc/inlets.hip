// Inlets, the device half (inlets.hpp; DESIGN.md section 3 "Inlets"): one kernel, one launch per step, for both solver families -- their per-face value buffers have
// the same [face][3] layout.  One lane per inlet face, 256-lane blocks, no atomics, no reduction:
//   k_inlet_values   U_f = a_0 S_0,f (+ a_1 S_1,f (+ a_2 S_2,f)), the step's a_m in the kernel arguments
// A streaming kernel of at most a few tens of thousands of faces (launch-latency bound): each lane reads up to three [f][3] shape vectors and stores one, consecutive
// lanes consecutive 24-byte records.  Every bracket is one IEEE operation (-ffp-contract=off), so a one-term inlet with a_0 = 1 stores its shape's bits.
#include <algorithm>

#include "device_util.hpp"
#include "inlets.hpp"

namespace fy {
namespace {

__global__ __launch_bounds__(256) void k_inlet_values(InletArgs A, int ne, const double* __restrict__ shapes, double* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    // the inlet this face belongs to: the last one whose first face is not past e (a static unroll: the arguments stay in scalar registers)
    int first = 0, base = 0, nt = 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int q = 0; q < FY_INLETS_MAX; ++q)
        if (q < A.n && e >= A.first[q]) { first = A.first[q]; base = A.base[q]; nt = A.nterms[q]; a0 = A.a[q][0]; a1 = A.a[q][1]; a2 = A.a[q][2]; }
    const double* s0 = shapes + 3 * (size_t)e;
    double u[3] = {a0 * s0[0], a0 * s0[1], a0 * s0[2]};
    if (nt > 1) { const double* s1 = s0 + 3 * (size_t)ne; for (int c = 0; c < 3; ++c) u[c] = u[c] + a1 * s1[c]; }
    if (nt > 2) { const double* s2 = s0 + 6 * (size_t)ne; for (int c = 0; c < 3; ++c) u[c] = u[c] + a2 * s2[c]; }
    double* o = out + 3 * (size_t)(base + (e - first));
    o[0] = u[0]; o[1] = u[1]; o[2] = u[2];
}

}  // namespace

int launch_inlet_values(hipStream_t s, const InletArgs& A, int ne, const double* shapes, double* out) {
    if (ne <= 0) return FY_OK;
    hipLaunchKernelGGL(k_inlet_values, dim3(div_up((size_t)ne, 256)), dim3(256), 0, s, A, ne, shapes, out);
    FY_LAUNCH_CHECK();
    return FY_OK;
}

}  // namespace fy
