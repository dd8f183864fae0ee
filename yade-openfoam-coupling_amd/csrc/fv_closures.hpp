// The finite-volume closures that the block solver (fv_kernels.hip in both its builds) and the general-mesh solver (ldu_kernels.hip) share: each stated ONCE, as a pure
// function of scalars (or of a const double* to a row-major 3 x 3 tensor) that knows neither solver's geometry or parameter structs.  A kernel loads or forms the operands
// the way its mesh has them (a wall distance, delta, a face weight, a wall-normal gradient) and calls; what differs between the solvers stays in the kernels.  The build
// has -ffp-contract=off, so one expression here is one sequence of FP64 operations in every kernel.  Everything is inlined into its caller: including this header adds no
// symbol to an object.  The arithmetic is OpenFOAM-6's, restated [OF-6]; oracle/fv_oracle.cpp and oracle/ldu_oracle.cpp restate it independently and include nothing of this.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/foamyade_hip.h"

namespace fy {
namespace {

// ------------------------------------------------------------------------------------------------ NVD / TVD limited convection
// [OF-6 LimitedScheme<vector, Limiter<NVDTVD>, limitFuncs::magSqr>, NVDTVD.H] one limiter per face from lPhi = magSqr(U).
// NVDTVD::r: gradf = lPhi_N - lPhi_P, gradcf = d . grad(lPhi)_C (C the upwind cell of the face flux, d = C_N - C_P); r = 2 gradcf / gradf - 1, with the sign-kept
// 1000-fold guard where gradf is small beside gradcf
__device__ __forceinline__ double nvd_r(double gradcf, double gradf) {
    if (fabs(gradcf) >= 1000.0 * fabs(gradf)) return 2.0 * 1000.0 * (gradcf >= 0 ? 1.0 : -1.0) * (gradf >= 0 ? 1.0 : -1.0) - 1.0;
    return 2.0 * (gradcf / gradf) - 1.0;
}
// the limiter of `scheme` (FY_CONVECTION_LIMITED_LINEAR .. FY_CONVECTION_QUICK) at r; twoByk = 2 / max(k, small) of limitedLinear k [OF-6 LimitedLinear.H, vanLeer.H, MUSCL.H,
// Minmod.H, SuperBee.H, QUICK.H].  The owner's weight is then limiter w_linear + (1 - limiter) pos0(flux) [limitedSurfaceInterpolationScheme::weights]
__device__ __forceinline__ double nvd_limiter(int scheme, double twoByk, double r) {
    switch (scheme) {
        case FY_CONVECTION_LIMITED_LINEAR: return fmax(fmin(twoByk * r, 1.0), 0.0);
        case FY_CONVECTION_VAN_LEER: return (r + fabs(r)) / (1.0 + fabs(r));
        case FY_CONVECTION_MUSCL: return fmax(fmin(fmin(2.0 * r, 0.5 * r + 0.5), 2.0), 0.0);
        case FY_CONVECTION_MINMOD: return fmax(fmin(fmin(r, 1.0), 2.0), 0.0);
        case FY_CONVECTION_SUPERBEE: return fmax(fmax(fmin(2.0 * r, 1.0), fmin(r, 2.0)), 0.0);
        // QUICK [OF-6 QUICK.H]: QLimiter = (phif - phiU) / (phiCD - phiU) with phif = (phiCD + phiU + (1 - w) d.grad(phi)_U) / 2, which is (3 + r) / 4 whatever the linear
        // weight w; limited "between upwind and downwind" only -- max(min(., 2), 0) -- so NOT a TVD limiter: it stays positive down to r = -3 and has no 2 r bound
        // (rounds 2 - 3 had min(2 r, .) here: another scheme under QUICK's name)
        default: return fmax(fmin((3.0 + r) / 4.0, 2.0), 0.0);
    }
}

// ------------------------------------------------------------------------------------------------ turbulence models
// LESModel Smagorinsky [OF-6 Smagorinsky.C: k(gradU), correctNut()] from T = grad U: D = symm(T); a = Ce / delta; b = 2/3 tr D; c = 2 Ck delta (dev D && D);
// k = sqr((-b + sqrt(b^2 + 4 a c)) / 2a); returns nut = Ck delta sqrt(k)
__device__ __forceinline__ double smagorinsky_nut(const double* T, double ck, double ce, double delta) {
    const double Dxx = T[0], Dyy = T[4], Dzz = T[8];
    const double Dxy = 0.5 * (T[1] + T[3]), Dxz = 0.5 * (T[2] + T[6]), Dyz = 0.5 * (T[5] + T[7]);
    const double trD = Dxx + Dyy + Dzz;
    const double a = ce / delta, b = (2.0 / 3.0) * trD, third = (1.0 / 3.0) * trD;
    // dev(D) && D over the nine components of the symmetric tensors
    const double dd = (Dxx - third) * Dxx + (Dyy - third) * Dyy + (Dzz - third) * Dzz + 2.0 * (Dxy * Dxy) + 2.0 * (Dxz * Dxz) + 2.0 * (Dyz * Dyz);
    const double cc = 2.0 * ck * delta * dd;
    const double r = (-b + sqrt(b * b + 4.0 * a * cc)) / (2.0 * a);
    return ck * delta * sqrt(r * r);
}
// the production's tensor part gradU && dev(twoSymm(gradU)) [OF-6 kEqn.C / kEpsilon.C correct(): G = nut (...)], T = grad U
__device__ __forceinline__ double production_tensor(const double* T) {
    const double tr2 = 2.0 * (T[0] + T[4] + T[8]);              // tr(twoSymm(T))
    double GG = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) GG += T[3 * a + b] * ((T[3 * a + b] + T[3 * b + a]) - (a == b ? (1.0 / 3.0) * tr2 : 0.0));
    return GG;
}
// correctNut() [OF-6 kEqn.C: nut = Ck sqrt(k) delta; kEpsilon.C: nut = Cmu sqr(k) / epsilon]; GeometricField::operator= assigns the `calculated` patches with the same
// expressions on the boundary values
__device__ __forceinline__ double nut_keqn(double ck, double k, double delta) { return ck * sqrt(k) * delta; }
__device__ __forceinline__ double nut_kepsilon(double cmu, double k, double eps) { return cmu * (k * k) / eps; }

// The transport equations' sources, X the cell's value of the field solved for (a = alpha, divU = fvc::div(phi)):  ... == Su - fvm::SuSp(c1, X) - fvm::Sp(c2, X)
struct TurbSource { double Su, c1, c2; };
// kEqn's k [OF-6 LES/kEqn/kEqn.C]: alpha G - fvm::SuSp(2/3 alpha divU, k) - fvm::Sp(Ce alpha sqrt(k) / delta, k)
__device__ __forceinline__ TurbSource keqn_k_source(double a, double G, double divU, double ce, double delta, double k) { return TurbSource{a * G, (2.0 / 3.0) * a * divU, ce * a * sqrt(k) / delta}; }
// kEpsilon's epsilon [OF-6 RAS/kEpsilon/kEpsilon.C]: C1 alpha G eps / k - fvm::SuSp((2/3 C1 - C3) alpha divU, eps) - fvm::Sp(C2 alpha eps / k, eps)
__device__ __forceinline__ TurbSource kepsilon_eps_source(double a, double G, double divU, double C1, double C2, double C3, double eps, double k) { return TurbSource{C1 * a * G * eps / k, ((2.0 / 3.0) * C1 - C3) * a * divU, C2 * a * eps / k}; }
// kEpsilon's k: alpha G - fvm::SuSp(2/3 alpha divU, k) - fvm::Sp(alpha eps / k, k)
__device__ __forceinline__ TurbSource kepsilon_k_source(double a, double G, double divU, double eps, double k) { return TurbSource{a * G, (2.0 / 3.0) * a * divU, a * eps / k}; }
// ... into the row of a cell of volume V [OF-6 fvm::SuSp: diag += V max(susp, 0), source -= V min(susp, 0) psi (implicit where it stabilises); fvm::Sp: diag += V sp;
// fvMatrix == volField: source += V field]
__device__ __forceinline__ void add_turb_source(const TurbSource& s, double V, double x, double& diag, double& source) {
    diag += V * (fmax(s.c1, 0.0) + s.c2);
    source += V * s.Su - V * fmin(s.c1, 0.0) * x;
}
// fvMatrix::relax of a scalar row without boundary coefficients [OF-6 fvMatrix.C]: D = max(|D|, sum |offdiag|) / factor, source += (D_new - D) psi
__device__ __forceinline__ void relax_scalar_row(double factor, double sum_mag_offdiag, double x, double& diag, double& source) {
    const double dn = fmax(fabs(diag), sum_mag_offdiag) / factor;
    source += (dn - diag) * x;
    diag = dn;
}
// the last step of bound(x, xMin) [OF-6 finiteVolume/cfdTools/general/bound/bound.C]: x = max(max(x, fvc::average(max(x, xMin)) pos0(-x)), xMin).  `average` matters only
// where pos0(-x) = 1; a caller that forms it only there passes x itself elsewhere
__device__ __forceinline__ double bound_value(double x, double average, double xMin) { return fmax(fmax(x, average), xMin); }

// ------------------------------------------------------------------------------------------------ wall functions
// nutkWallFunction [OF-6 nutkWallFunctionFvPatchScalarField::nut]: y+ = Cmu^1/4 y sqrt(k_P) / nu; nut_w = nu (y+ kappa / ln(E y+) - 1) above yPlusLam (common.hpp:
// wall_yplus_lam), else 0.  y: the wall distance of the cell centre
__device__ __forceinline__ double nutk_wall_nut(double cmu25, double y, double k, double nu, double yPlusLam, double kappa, double E) {
    const double yPlus = cmu25 * y * sqrt(k) / nu;
    return yPlus > yPlusLam ? nu * (yPlus * kappa / log(E * yPlus) - 1.0) : 0.0;
}
// epsilonWallFunction::calculate [OF-6 epsilonWallFunctionFvPatchScalarField.C], the terms of ONE wall face; a cell's epsilon and G are their averages over its wall faces
// (cornerWeights = 1 / number of wall faces).  epsilon: Cmu^3/4 k^3/2 / (kappa y)
__device__ __forceinline__ double wall_epsilon_term(double cmu75, double k, double kappa, double y) { return cmu75 * pow(k, 1.5) / (kappa * y); }
// G: (nut_w + nu) |snGrad U| Cmu^1/4 sqrt(k) / (kappa y)
__device__ __forceinline__ double wall_G_term(double nutw, double nu, double magGradUw, double cmu25, double k, double kappa, double y) { return (nutw + nu) * magGradUw * cmu25 * sqrt(k) / (kappa * y); }

}  // namespace
}  // namespace fy
