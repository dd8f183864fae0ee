// k_field_average: the running mean / second central moment update of fy::FieldAverage (field_average.hpp), one launch per step for all items.
// A pure streaming kernel: every value is read once and written once, no atomics, no LDS, no reduction.  blockIdx.y selects the item; an item's share of
// the row's blocks (AvgEntry::nblk, by its traffic) strides over its work.  Scalar items and vector items without prime2Mean are flat arrays: two values per
// thread, 16-byte accesses.  A vector item with prime2Mean takes two cells per thread: x and m as three 16-byte accesses each, the twelve P values as six.
// Built with -ffp-contract=off like every kernel here: each line below is one IEEE operation, which is what makes the result reproducible bit for bit
// against a restatement that performs the same operations (tests/field_average_ref.py).
#include "field_average.hpp"

namespace fy {

namespace {

// one value of a scalar field, or one component of a mean-only vector field
__device__ __forceinline__ void avg_value(double x, double& m, double& P, double a, double b, bool with_P) {
    if (with_P) P = P + m * m;
    const double mn = a * m + b * x;
    if (with_P) P = (a * P + b * (x * x)) - mn * mn;
    m = mn;
}

// one cell of a vector field with prime2Mean: P in symmTensor order xx xy xz yy yz zz
__device__ __forceinline__ void avg_vector_cell(const double x[3], double m[3], double P[6], double a, double b) {
    int q = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++q) P[q] = P[q] + m[i] * m[j];
    double mn[3];
    for (int i = 0; i < 3; ++i) mn[i] = a * m[i] + b * x[i];
    q = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++q) P[q] = (a * P[q] + b * (x[i] * x[j])) - mn[i] * mn[j];
    for (int i = 0; i < 3; ++i) m[i] = mn[i];
}

__device__ __forceinline__ void avg_vector_cell_at(const AvgEntry& e, size_t c) {
    double x[3], m[3], P[6];
    for (int i = 0; i < 3; ++i) { x[i] = e.x[3 * c + i]; m[i] = e.m[3 * c + i]; }
    for (int q = 0; q < 6; ++q) P[q] = e.P[6 * c + q];
    avg_vector_cell(x, m, P, e.a, e.b);
    for (int i = 0; i < 3; ++i) e.m[3 * c + i] = m[i];
    for (int q = 0; q < 6; ++q) e.P[6 * c + q] = P[q];
}

__global__ __launch_bounds__(256) void k_field_average(const AvgTable tab, size_t n_cells) {
    const AvgEntry e = tab.e[blockIdx.y];
    if ((int)blockIdx.x >= e.nblk) return;
    const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)e.nblk * 256;
    const double a = e.a, b = e.b;
    const bool with_P = e.P != nullptr;
    if (e.mode == 0) {
        const size_t total = n_cells * (size_t)e.comp, pairs = total / 2;
        const double2* x2 = reinterpret_cast<const double2*>(e.x);
        double2* m2 = reinterpret_cast<double2*>(e.m);
        double2* P2 = reinterpret_cast<double2*>(e.P);
        for (size_t t = t0; t < pairs; t += stride) {
            const double2 x = x2[t];
            double2 m = m2[t], P = with_P ? P2[t] : double2{0.0, 0.0};
            avg_value(x.x, m.x, P.x, a, b, with_P);
            avg_value(x.y, m.y, P.y, a, b, with_P);
            m2[t] = m;
            if (with_P) P2[t] = P;
        }
        if ((total & 1) && t0 == 0) {                  // the odd value at the end
            double m = e.m[total - 1], P = with_P ? e.P[total - 1] : 0.0;
            avg_value(e.x[total - 1], m, P, a, b, with_P);
            e.m[total - 1] = m;
            if (with_P) e.P[total - 1] = P;
        }
    } else if (e.mode == 1) {
        const size_t total = n_cells * (size_t)e.comp;
        for (size_t t = t0; t < total; t += stride) {
            double m = e.m[t], P = with_P ? e.P[t] : 0.0;
            avg_value(e.x[t], m, P, a, b, with_P);
            e.m[t] = m;
            if (with_P) e.P[t] = P;
        }
    } else if (e.mode == 2) {
        const size_t pairs = n_cells / 2;
        const double2* x2 = reinterpret_cast<const double2*>(e.x);
        double2* m2 = reinterpret_cast<double2*>(e.m);
        double2* P2 = reinterpret_cast<double2*>(e.P);
        for (size_t t = t0; t < pairs; t += stride) {
            double2 xv[3], mv[3], Pv[6];
            for (int i = 0; i < 3; ++i) { xv[i] = x2[3 * t + i]; mv[i] = m2[3 * t + i]; }
            for (int q = 0; q < 6; ++q) Pv[q] = P2[6 * t + q];
            double xa[3] = {xv[0].x, xv[0].y, xv[1].x}, xb[3] = {xv[1].y, xv[2].x, xv[2].y};
            double ma[3] = {mv[0].x, mv[0].y, mv[1].x}, mb[3] = {mv[1].y, mv[2].x, mv[2].y};
            double Pa[6] = {Pv[0].x, Pv[0].y, Pv[1].x, Pv[1].y, Pv[2].x, Pv[2].y}, Pb[6] = {Pv[3].x, Pv[3].y, Pv[4].x, Pv[4].y, Pv[5].x, Pv[5].y};
            avg_vector_cell(xa, ma, Pa, a, b);
            avg_vector_cell(xb, mb, Pb, a, b);
            m2[3 * t] = double2{ma[0], ma[1]}; m2[3 * t + 1] = double2{ma[2], mb[0]}; m2[3 * t + 2] = double2{mb[1], mb[2]};
            for (int q = 0; q < 3; ++q) { P2[6 * t + q] = double2{Pa[2 * q], Pa[2 * q + 1]}; P2[6 * t + 3 + q] = double2{Pb[2 * q], Pb[2 * q + 1]}; }
        }
        if ((n_cells & 1) && t0 == 0) avg_vector_cell_at(e, n_cells - 1);
    } else {
        for (size_t c = t0; c < n_cells; c += stride) avg_vector_cell_at(e, c);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int launch_field_average(hipStream_t stream, const AvgTable& tab_in, int n_items, size_t n_cells) {
    if (n_items < 1 || n_cells == 0) return FY_OK;
    AvgTable tab = tab_in;
    // doubles moved per cell (x read; m and P read and written), and the threads an item can use
    double traffic[FY_AVERAGE_MAX_ITEMS], total = 0.0;
    size_t work[FY_AVERAGE_MAX_ITEMS];
    for (int q = 0; q < n_items; ++q) {
        AvgEntry& e = tab.e[q];
        const bool al = aligned16(e.x) && aligned16(e.m) && aligned16(e.P);
        const bool vecP = e.comp == 3 && e.P;
        e.mode = vecP ? (al ? 2 : 3) : (al ? 0 : 1);
        traffic[q] = (double)(3 * e.comp + (e.P ? (e.comp == 3 ? 12 : 2) : 0));
        total += traffic[q];
        const size_t units = vecP ? n_cells : n_cells * (size_t)e.comp;
        work[q] = (e.mode == 0 || e.mode == 2) ? (units + 1) / 2 : units;
    }
    // ~2048 blocks in all (8 per CU), grid-stride the rest; each item takes its share by traffic
    unsigned gx = 1;
    for (int q = 0; q < n_items; ++q) {
        const size_t need = (work[q] + 255) / 256;
        size_t share = (size_t)(2048.0 * traffic[q] / total + 0.5);
        share = std::max<size_t>(1, std::min(share, need));
        tab.e[q].nblk = (int)share;
        gx = std::max(gx, (unsigned)share);
    }
    hipLaunchKernelGGL(k_field_average, dim3(gx, (unsigned)n_items), dim3(256), 0, stream, tab, n_cells);
    FY_HIP(hipGetLastError());
    return FY_OK;
}

}  // namespace fy
