// fy::SolidStats (solid_stats.hpp): host code that sequences the kernels of particle_moments.hip, for both solvers.
#include "solid_stats.hpp"

#include "particle_kernels.hpp"

namespace fy {

int SolidStats::set(bool enable, size_t n_cells, bool thermal, hipStream_t stream) {
    sums.release(); fields.release(); out8.release();
    on = false;
    if (!enable) return FY_OK;
    n = n_cells; with_T = thermal;
    FY_TRY(sums.alloc_exact(8 * n));
    FY_TRY(fields.alloc_exact((with_T ? 8 : 7) * n));
    FY_HIP(hipMemsetAsync(sums.p, 0, sums.n * sizeof(double), stream));
    FY_HIP(hipMemsetAsync(fields.p, 0, fields.n * sizeof(double), stream));
    FY_HIP(hipStreamSynchronize(stream));
    on = true;
    return FY_OK;
}

int SolidStats::pass(Coupling& C, hipStream_t stream, CellWindow cw, const double* vol, HeatExchange* he, bool bucketed) {
    clock.begin(stream);
    FY_HIP(hipMemsetAsync(sums.p, 0, sums.n * sizeof(double), stream));      // cleared by the pass itself, not by setSourceZero: the sums run over all batches
    const SolidMoments m = moments();
    for (int bi = 0; bi < C.n_batches; ++bi) {
        Batch& b = *C.batches[(size_t)bi];
        if (b.n == 0) continue;
        // the temperatures the heat exchange holds for this batch now: the array the library integrates or the caller's, else the uniform value
        const double* tp = nullptr;
        double tp_uniform = 0.0;
        if (he && he->on) {
            tp_uniform = he->hp.tp_uniform;
            if ((size_t)bi < he->pb.size() && he->pb[(size_t)bi]->has_tp && he->pb[(size_t)bi]->tp_n == b.n) tp = he->pb[(size_t)bi]->Tp.p;
        }
        if (C.gaussian) {
            TileBuckets tb{};
            if (bucketed) {
                // the momentum back-scatter's buckets with the capacities formed from this step's own demand, as HeatExchange::coefficients takes them (which, when on,
                // has finished with them: same stream); the pass changes no capacity and leaves every demand counter at zero
                tb = C.buckets_of(b, 1);
                if (!tb.cell || !b.caps_ready || !b.ev_caps || b.caps_key != (const void*)C.buckets_of(b, 0).off)
                    return fail(FY_ERR_INVALID, "%s_step: solid statistics: batch %d has no tile-bucket capacities of this step (a Gaussian batch on a structured block always has)", who, bi);
                FY_HIP(hipStreamWaitEvent(stream, b.ev_caps, 0));
            }
            FY_TRY(launch_moments_gaussian(stream, C.soa_of(b), b.n, cw, tp, tp_uniform, m, tb));
        } else {
            FY_TRY(launch_moments_point(stream, b.d_rec, b.n, b.incell.p, cw, tp, tp_uniform, m));
        }
    }
    FY_TRY(launch_solid_stats_cells(stream, (int64_t)n, m, vol, views()));
    clock.end(stream);
    return FY_OK;
}

namespace {
const char* const kSolidNames[] = {"nParticle", "solidFraction", "uSolid", "granularTemperature", "dSauter", "TParticle"};
}

bool SolidStats::is_name(const std::string& name) {
    if (name == "solidMoments") return true;
    for (const char* k : kSolidNames) if (name == k) return true;
    return false;
}

const double* SolidStats::source(const std::string& name, int* comp) const {
    if (!on) return nullptr;
    const SolidFields f = views();
    const double* const p[] = {f.nParticle, f.solidFraction, f.uSolid, f.granularTemperature, f.dSauter, f.TParticle};
    for (int q = 0; q < 6; ++q)
        if (name == kSolidNames[q] && p[q]) { *comp = q == 2 ? 3 : 1; return p[q]; }
    return nullptr;
}

int SolidStats::field(const std::string& name, hipStream_t stream, double** ptr, size_t* count) {
    if (!on) return fail(FY_ERR_INVALID, "%s field '%s' does not exist while the solid statistics are off (%s_set_solid_statistics)", who, name.c_str(), who);
    if (name == "solidMoments") {
        if (!out8.p) FY_TRY(out8.alloc_exact(8 * n));
        FY_TRY(launch_moments_interleave(stream, (int64_t)n, moments(), out8.p));
        *ptr = out8.p; *count = 8 * n;
        return FY_OK;
    }
    int comp = 0;
    const double* p = source(name, &comp);
    if (!p) return fail(FY_ERR_INVALID, "%s field '%s' does not exist in this case (heat transfer is off)", who, name.c_str());
    *ptr = const_cast<double*>(p); *count = (size_t)comp * n;
    return FY_OK;
}

}  // namespace fy
