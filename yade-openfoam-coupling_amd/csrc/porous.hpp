// Porous zones (fy_porous_desc; DESIGN.md section 3 "Porous zones", DESIGN_FV.md "Porous resistance"): a Darcy-Forchheimer resistance, diagonal in the global axes and
// implicit per component, in the cells of up to FY_POROUS_MAX_ZONES zones.  Shared by fy_solver and fy_ldu_solver:
//   PorousDev         the device record the momentum assembly kernels read through ONE extra pointer argument (null: no zones, every kernel takes the path it took
//                     before): the cell-to-zone map (one byte per cell, 0 = none) and the coefficients
//   porous_diag()     the one statement of the coefficient a V C_q, which the three assembly kernels and k_porous_force share
//   Porous            the host side: validation, the map, the compact cell list k_porous_force runs over, the statistics
// The step launches nothing for the zones and never waits for them; k_porous_force (porous.hip) runs on request only.
#pragma once
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "common.hpp"

namespace fy {

struct PorousDev {
    const unsigned char* zone_of;                 // [cells] 0: none, 1 + zone otherwise
    double d[FY_POROUS_MAX_ZONES][3];             // Darcy [1/m^2]
    double f[FY_POROUS_MAX_ZONES][3];             // Forchheimer [1/m]
};

#ifdef __HIPCC__
// a V C_q of zone z (0-based) at velocity u: C_q = nu d_q + (0.5 |u|) f_q, |u| = sqrt((u0^2 + u1^2) + u2^2); every bracket one IEEE operation (-ffp-contract=off)
__device__ __forceinline__ void porous_diag(const PorousDev* __restrict__ por, int z, double nu, double aV, double u0, double u1, double u2, double (&pc)[3]) {
    const double hm = 0.5 * sqrt((u0 * u0 + u1 * u1) + u2 * u2);
#pragma unroll
    for (int q = 0; q < 3; ++q) pc[q] = aV * (nu * por->d[z][q] + hm * por->f[z][q]);
}
// the same for owned cell t of a sweep: false outside the zones (one byte read), else pc = a V C_q(u), u = the cell's three velocity components
__device__ __forceinline__ bool porous_cell(const PorousDev* __restrict__ por, int t, double nu, double aV, const double* __restrict__ u, double (&pc)[3]) {
    const int pz = por->zone_of[t];
    if (!pz) return false;
    porous_diag(por, pz - 1, nu, aV, u[0], u[1], u[2], pc);
    return true;
}
// the component maximum of the same, for fvMatrix::relax's dominance test: 0 outside the zones.  a V >= 0 and rounding is monotone, so a V max_q C_q has the bits of
// max_q (a V C_q); formed as a running maximum to keep the registers it needs few
__device__ __forceinline__ double porous_cell_max(const PorousDev* __restrict__ por, int t, double nu, double aV, const double* __restrict__ u) {
    const int pz = por->zone_of[t];
    if (!pz) return 0.0;
    const double hm = 0.5 * sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    double m = nu * por->d[pz - 1][0] + hm * por->f[pz - 1][0];
    m = fmax(m, nu * por->d[pz - 1][1] + hm * por->f[pz - 1][1]);
    m = fmax(m, nu * por->d[pz - 1][2] + hm * por->f[pz - 1][2]);
    return aV * m;
}
#endif

constexpr int kPorousSums = 5;      // per zone: S V, S a V, S a V C_q U_q (q = 0, 1, 2)

// the compact list is padded per zone to whole 256-lane blocks (-1: no cell), so a block serves one zone (blk_zone; -1: a padding block of the reduction grid) and leaves
// its kPorousSums partials in that zone's slots; the other zones' slots at its place stay zero from the set-up.  vol: the cell volumes, entry by entry.
// U, alpha: the OWNED cells' arrays (alpha null: a = 1)
int launch_porous_force(hipStream_t s, int n_padded, const int32_t* cells, const int32_t* blk_zone, const double* vol, const PorousDev* por, double nu, const double* U,
                        const double* alpha, double* partials);
int launch_porous_zone_f64(hipStream_t s, int n, const unsigned char* zone_of, double* out);

struct Porous {
    int n_zones = 0;
    std::vector<std::string> names;
    std::vector<int64_t> counts;
    int n_padded = 0;
    DevBuf<unsigned char> zone_of;
    DevBuf<PorousDev> rec;
    DevBuf<int32_t> cells, blk_zone;
    DevBuf<double> vol, partials, sums, f64;
    KernelClock clock;                            // "porous_force"
    ~Porous() { clock.destroy(); }
    bool on() const { return n_zones > 0; }
    const PorousDev* dev() const { return n_zones > 0 ? rec.p : nullptr; }
    void off() {
        n_zones = 0; n_padded = 0; names.clear(); counts.clear();
        zone_of.release(); rec.release(); cells.release(); blk_zone.release(); vol.release(); partials.release(); sums.release(); f64.release();
    }
    // d null or n_zones == 0: off.  volume(c): V of solver cell c.  The new set is built beside the old one and traded in after the stream is drained (a step in flight
    // may still read the record this call replaces): a call that fails -- a refusal, an allocation, a copy -- leaves what was set as it was
    int configure(const fy_porous_desc* d, int n_cells, hipStream_t stream, const char* who, const std::function<double(int)>& volume);
    // the four arrays per zone (any may be null); waits for the device
    int stats(hipStream_t stream, const char* who, double nu, const double* U, const double* alpha, int32_t* nz, int64_t* cnt, double* volume, double* void_volume, double* force);
    int zone_field(hipStream_t stream, int n_cells, double** ptr, size_t* count);
};

}  // namespace fy
