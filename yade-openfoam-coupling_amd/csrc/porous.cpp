// Porous zones, host side (porous.hpp): the setter's validation, the cell-to-zone map, the compact list of k_porous_force and the statistics
#include "porous.hpp"

#include "fv_linalg_kernels.hpp"

namespace fy {

int Porous::configure(const fy_porous_desc* d, int n_cells, hipStream_t stream, const char* who, const std::function<double(int)>& volume) {
    if (!d || d->n_zones == 0) {
        FY_HIP(hipStreamSynchronize(stream));
        off();
        return FY_OK;
    }
    if (d->n_zones < 0 || d->n_zones > FY_POROUS_MAX_ZONES)
        return fail(FY_ERR_INVALID, "%s: %d porous zones (1 to FY_POROUS_MAX_ZONES = %d)", who, d->n_zones, FY_POROUS_MAX_ZONES);
    std::vector<unsigned char> map((size_t)n_cells, 0);
    std::vector<std::string> nm;
    PorousDev h{};
    for (int z = 0; z < d->n_zones; ++z) {
        const fy_porous_zone& Z = d->zones[z];
        const std::string name(Z.name, strnlen(Z.name, sizeof(Z.name)));
        const char* zn = name.empty() ? "(unnamed)" : name.c_str();
        for (int q = 0; q < 3; ++q) {
            if (!std::isfinite(Z.d[q]) || Z.d[q] < 0) return fail(FY_ERR_INVALID, "%s: porous zone '%s': d[%d] = %g (a Darcy coefficient is finite and >= 0, in 1/m^2)", who, zn, q, Z.d[q]);
            if (!std::isfinite(Z.f[q]) || Z.f[q] < 0) return fail(FY_ERR_INVALID, "%s: porous zone '%s': f[%d] = %g (a Forchheimer coefficient is finite and >= 0, in 1/m)", who, zn, q, Z.f[q]);
            h.d[z][q] = Z.d[q]; h.f[z][q] = Z.f[q];
        }
        if (Z.n_cells <= 0) return fail(FY_ERR_INVALID, "%s: porous zone '%s' is empty (n_cells = %d)", who, zn, Z.n_cells);
        if (!Z.cells) return fail(FY_ERR_INVALID, "%s: porous zone '%s': null cell list", who, zn);
        for (int e = 0; e < Z.n_cells; ++e) {
            const int c = Z.cells[e];
            if (c < 0 || c >= n_cells) return fail(FY_ERR_INVALID, "%s: porous zone '%s': cell label %d out of range (the mesh has %d cells)", who, zn, c, n_cells);
            if (map[(size_t)c]) {
                const int o = map[(size_t)c] - 1;
                if (o == z) return fail(FY_ERR_INVALID, "%s: porous zone '%s' lists cell %d twice", who, zn, c);
                return fail(FY_ERR_INVALID, "%s: cell %d is in two porous zones ('%s' and '%s')", who, c, nm[(size_t)o].c_str(), zn);
            }
            map[(size_t)c] = (unsigned char)(z + 1);
        }
        nm.push_back(zn);
    }
    // the compact list: zone by zone, ascending cell label, each zone padded to whole blocks
    std::vector<int32_t> list, bz;
    std::vector<double> v;
    std::vector<int64_t> cnt((size_t)d->n_zones, 0);
    for (int z = 0; z < d->n_zones; ++z) {
        for (int c = 0; c < n_cells; ++c)
            if (map[(size_t)c] == z + 1) { list.push_back(c); v.push_back(volume(c)); ++cnt[(size_t)z]; }
        while (list.size() % 256) { list.push_back(-1); v.push_back(0.0); }
        bz.resize(list.size() / 256, z);
    }
    const int np = (int)list.size(), stride = red_blocks(np);
    bz.resize((size_t)stride, -1);
    // the new set is built in buffers of its own and traded in only when all of it is on the device: an allocation or a copy that fails leaves the zones that were
    // set (or none) as they were, like a refusal above, and frees what it had allocated (the temporaries' destructors)
    DevBuf<unsigned char> t_zone;
    DevBuf<PorousDev> t_rec;
    DevBuf<int32_t> t_cells, t_blk;
    DevBuf<double> t_vol, t_part, t_sums;
    FY_TRY(t_zone.alloc_exact(map.size())); FY_TRY(t_rec.alloc_exact(1)); FY_TRY(t_cells.alloc_exact(list.size())); FY_TRY(t_blk.alloc_exact(bz.size()));
    FY_TRY(t_vol.alloc_exact(v.size())); FY_TRY(t_part.alloc_exact((size_t)kPorousSums * d->n_zones * stride)); FY_TRY(t_sums.alloc_exact((size_t)kPorousSums * d->n_zones));
    h.zone_of = t_zone.p;
    FY_HIP(hipMemcpy(t_zone.p, map.data(), map.size(), hipMemcpyHostToDevice));
    FY_HIP(hipMemcpy(t_rec.p, &h, sizeof(h), hipMemcpyHostToDevice));
    FY_HIP(hipMemcpy(t_cells.p, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    FY_HIP(hipMemcpy(t_blk.p, bz.data(), bz.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    FY_HIP(hipMemcpy(t_vol.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    FY_HIP(hipMemset(t_part.p, 0, t_part.n * sizeof(double)));      // a block writes its own zone's slots only: the rest stays zero
    FY_HIP(hipStreamSynchronize(stream));                           // a step in flight may still read the record this call replaces
    auto trade = [](auto& a, auto& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); };
    trade(zone_of, t_zone); trade(rec, t_rec); trade(cells, t_cells); trade(blk_zone, t_blk); trade(vol, t_vol); trade(partials, t_part); trade(sums, t_sums);
    f64.release();
    n_zones = d->n_zones; n_padded = np; names = nm; counts = cnt;
    return FY_OK;
}

int Porous::stats(hipStream_t stream, const char* who, double nu, const double* U, const double* alpha, int32_t* nz, int64_t* cnt, double* volume, double* void_volume, double* force) {
    if (!on()) return fail(FY_ERR_INVALID, "%s: no porous zone is set", who);
    clock.begin(stream);
    FY_TRY(launch_porous_force(stream, n_padded, cells.p, blk_zone.p, vol.p, rec.p, nu, U, alpha, partials.p));
    FY_TRY(launch_reduce_finalize(stream, partials.p, n_padded, kPorousSums * n_zones, nullptr, sums.p));
    clock.end(stream);
    std::vector<double> h((size_t)kPorousSums * n_zones);
    FY_HIP(hipMemcpyAsync(h.data(), sums.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    FY_HIP(hipStreamSynchronize(stream));
    clock.collect();
    if (nz) *nz = n_zones;
    for (int z = 0; z < n_zones; ++z) {
        if (cnt) cnt[z] = counts[(size_t)z];
        if (volume) volume[z] = h[(size_t)kPorousSums * z];
        if (void_volume) void_volume[z] = h[(size_t)kPorousSums * z + 1];
        if (force) for (int q = 0; q < 3; ++q) force[3 * z + q] = h[(size_t)kPorousSums * z + 2 + q];
    }
    return FY_OK;
}

int Porous::zone_field(hipStream_t stream, int n_cells, double** ptr, size_t* count) {
    if (!f64.p) FY_TRY(f64.alloc_exact((size_t)n_cells));
    FY_TRY(launch_porous_zone_f64(stream, n_cells, zone_of.p, f64.p));
    *ptr = f64.p; *count = (size_t)n_cells;
    return FY_OK;
}

}  // namespace fy
