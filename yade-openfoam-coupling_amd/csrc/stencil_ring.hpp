// What the particle kernel sources share per particle (particle_bin.hip, particle_locate.hip, particle_force.hip, particle_heat.hip): the stencil ring's
// addressing, the unnormalised Gaussian weight, the particle volume's cube and the z-slab ownership test.  Device only; everything here is inlined
// into its caller: including this header adds no symbol to an object.
#pragma once
#include <hip/hip_runtime.h>

#include "particle_kernels.hpp"

namespace fy {
namespace {

// pow(dia, 3.0) of FoamYade.H:36 as two multiplications in the two hot kernels (k_locate_deposit, k_force_gaussian): the library pow is ~200 FP64
// instructions per call, which showed in the VALU-bound list scan (1.02 -> 0.98 ms); x*x*x is within one ulp of the correctly rounded cube, the
// same order as the difference between the device's and glibc's pow that the golden tolerances already carry.  The cold sites keep pow: with
// the cheap form the compiler if-converts the opt-in torque branch of force_law and the force kernel loses 0.2 ms to register pressure
__device__ __forceinline__ double cube3(double x) { return (x * x) * x; }

// ------------------------------------------------------------------------------------------------ the stencil ring
// A particle's stencil rows (ParticleSoA::ids, ::w: [kMaxK][cap]) are a ring indexed by push order: the walk's or the list scan's push number `push`
// lives in row push & 15 of column i.
__device__ __forceinline__ size_t stencil_slot(const ParticleSoA& p, int64_t i, int push) { return (size_t)(push & (kMaxK - 1)) * p.cap + (size_t)i; }

// chain = pushes so far (chain_len[i]); the ring keeps the k = min(chain, 16) newest, pushes first .. chain - 1.  The two orders they are walked in:
//   * OLDEST FIRST, push first + t (the force and heat passes, k_locate_deposit's normalisation): row (first + t) & 15 is row t for every chain that
//     never wrapped (chain <= 12: all of them in practice) -- so in iteration t all lanes of a wave read the same row, whatever their chain lengths,
//     and the id / weight loads are coalesced (newest first spreads each load over as many rows as the wave has chain lengths: ~8).  The sums are the
//     reference's sums taken in the opposite order (FoamYade.C:358-365 runs over the container newest first); the difference is rounding in the last
//     bits (covered by the 1e-10 bar of the golden tests);
//   * LAST PUSH FIRST, push chain - 1 - t (the weight sums of walk_deposit and k_deposit, k_unpack_stencils' rows): ascending squared distance, the
//     order calcInterpWeightGaussian adds the weights in (FoamYade.C:301-311) -- allwt is the reference's sum, addition for addition.
struct StencilSpan { int chain, k, first; };
__device__ __forceinline__ StencilSpan stencil_span(int chain) {
    const int k = chain < kMaxK ? chain : kMaxK;
    return StencilSpan{chain, k, chain - k};
}

// the unnormalised weight of a cell centre at squared distance d2, FoamYade.C:308 (reciprocal instead of the division: an ulp, inside the weights' 1e-10
// bar).  One statement for the list scan, the walk's own deposit and k_deposit: a particle's weights do not depend on which path placed it
__device__ __forceinline__ double gauss_wu(const GaussParams& gp, double d2) { return exp(-d2 * (1.0 / gp.two_sigma2)) * gp.range_cu * gp.sigma_pi; }

// ------------------------------------------------------------------------------------------------ z-slab ownership
// may this record be located here: its containing cell lies in the slab's planes and -- records that came in wire pieces -- in its piece's layers
__device__ __forceinline__ bool own_planes(const SlabOwn& own, int wire_index, int kz, double qx, double qy, double qz) {
    if (kz < own.k0 || kz >= own.k1) return false;
    if (own.npieces == 0) return true;
    const double qa = own.paxis == 0 ? qx : (own.paxis == 1 ? qy : qz);
    int ka = (int)floor((qa - own.po) / own.dx);
    ka = min(max(ka, 0), own.pn - 1);
    int a0 = 0, a1 = 0;
    for (int q = 0; q < own.npieces; ++q)
        if (wire_index >= own.pstart[q]) { a0 = own.pk0[q]; a1 = own.pk1[q]; }
    return ka >= a0 && ka < a1;
}

}  // namespace
}  // namespace fy
