// Launcher declarations of fv_kernels.hip -- included by fv_kernels.hpp once per geometry model (namespaces fy and fy::gr); no include guard on purpose.
// Every launcher here takes an FvGeo; the geometry-free ones (pressure solver, multigrid, vector kernels) are declared once, in fv_linalg_kernels.hpp.
// Reducing kernels write per-block partials to partials[slot * red_blocks(Nc) + block]; launch_reduce_finalize folds them in a fixed order.

// ---- field operators
int launch_flux_of(hipStream_t s, FvGeo g, const double* F, Face3 out);                                   // fvc::flux(F), createPhi
int launch_courant(hipStream_t s, FvGeo g, CFace3 phi, double* partials);                                  // slots 0 (max) 1 (sum)
// Gout != nullptr: also emit the laminar stress tensor alpha nu dev2(T(grad U)); write_vgrad = 0 skips the vGrad store,
// write_pfields = 0 skips gradP / divT (pimple only); ddtU != nullptr: also ddtU_f = fvc::div(phi, U) (pimpleFoamYade.C:73)
int launch_pre_coupling(hipStream_t s, FvGeo g, const double* U, const double* p, const double* alpha, CFace3 psn,
                        double* vGrad, double* gradP, double* divT, double* Gout, int write_vgrad, int write_pfields,
                        CFace3 phi = CFace3{}, double* ddtU = nullptr, double* Uold_out = nullptr,
                        double* cellrec = nullptr /* pimple + write_pfields: also the force pass's 64-byte cell records (what launch_pack_cells builds) */,
                        double rec_nu = 0.0, double rec_rhoF = 0.0,
                        Face3 dcorr = Face3{} /* with phi = phi.oldTime() and U = U.oldTime(): the old-time part of ddtCorr per face, coef / deltaT (phi.old - flux(U.old)) */);
int launch_interp_alpha(hipStream_t s, FvGeo g, const double* alpha, Face3 alphaf);
// G: three vec3 fields (rows of the tensor) over the whole storage, as k_pre_coupling writes them
int launch_div_G(hipStream_t s, FvGeo g, const double* G, double* divG);
// the same divG straight from U and alpha (and g.nut): launch_pre_coupling(Gout) + launch_div_G in one sweep over 3-D tiles, G held in LDS.  Single domain only
int launch_stress_div(hipStream_t s, FvGeo g, const double* U, const double* alpha, double* divG);
// The transport equations of the two-equation / one-equation closures (DPMTurbulenceModels.C:70-71 RAS kEpsilon, :76-77 LES kEqn):
//   fvm::ddt(alpha, X) + fvm::div(alphaPhi, X) - fvm::laplacian(alpha (nut / sigma + nu), X) == Su - fvm::SuSp(c1, X) - fvm::Sp(c2, X)
// mode 0  kEqn      X = k:    Su = alpha G,            c1 = 2/3 alpha divU,            c2 = Ce alpha sqrt(k) / delta          (sigma = 1)
// mode 1  kEpsilon  X = eps:  Su = C1 alpha G eps / k,  c1 = (2/3 C1 - C3) alpha divU,  c2 = C2 alpha eps / k                  (sigma = sigmaEps)
// mode 2  kEpsilon  X = k:    Su = alpha G,            c1 = 2/3 alpha divU,            c2 = alpha eps / k  (eps already new)  (sigma = sigmak)
// with G = nut (gradU && dev(twoSymm(gradU))), divU = fvc::div(phi).  bc / val: boundary conditions of X (0 zeroGradient, 1 fixedValue);
// upwind: convection scheme of X (0 Gauss linear, 1 Gauss upwind); relax: relaxation factor of the equation (<= 0: none); xmin: bound()
// wall[p] = 1: patch p carries epsilonWallFunction [OF-6 epsilonWallFunctionFvPatchScalarField.C]: in the cells next to it
//   eps = Cmu^3/4 k^3/2 / (kappa y) is IMPOSED (fvMatrix::setValues: the row becomes diag x = diag value, the neighbours' coefficients towards the
//   cell move to their sources) and the production G of both equations is replaced by the corner-weighted wall value
//   (1/W) sum_faces (nut_w + nu) |snGrad U| Cmu^1/4 sqrt(k) / (kappa y)
// assembles the equation into the momentum matrix's storage (free after the correctors) as a 3-component system whose components 1, 2 are
// identically zero, so that the momentum solver's Jacobi pass solves it: x3 = {X, 0, 0}, b3 = {source, 0, 0}
int launch_assemble_turb(hipStream_t s, FvGeo g, TurbEqn e, const double* k, const double* eps, const double* alpha, CFace3 alphaf, CFace3 phi,
                         const double* vGrad, const double* U, Mom7 M, double* b3, double* x3);
// bound(X, xmin) [OF-6 bound.C] on the solved component 0 of x3 -> X; nut_mode 1: nut = Ck sqrt(k) delta (kEqn::correctNut, X = k),
// 2: nut = Cmu k^2 / eps (kEpsilon::correctNut, X = k, eps given), 0: leave nut alone (the epsilon equation)
int launch_turb_finish(hipStream_t s, FvGeo g, TurbEqn e, const double* x3, double* X, int nut_mode, double cmu, const double* eps, double* nut);
// The fluid temperature equation (fy_thermal_desc), assembled like the turbulence transport equations into the momentum matrix's storage (x3 = {T, 0, 0}, b3 = {source, 0, 0}):
//   alpha V (T - T_old) / dt + sum_f F_f T_f - T sum_f F_f - sum_f alpha_f Deff_f |S_f| / |d_f| (T_N - T) = (Su - Sp T) / (rho_f cp),  F_f = alpha_f phi_f, Deff = D + nut / Prt
// alpha == nullptr: alpha = 1 (icoFoamYade); Sp == nullptr: no particle sources.  launch_scalar_finish copies the solved component 0 back to the field
int launch_assemble_scalar(hipStream_t s, FvGeo g, ScalarEqn e, const double* T, const double* alpha, CFace3 phi, const double* Sp, const double* Su, Mom7 M,
                           double* b3, double* x3);
int launch_scalar_finish(hipStream_t s, FvGeo g, const double* x3, double* X);
int launch_smagorinsky_nut(hipStream_t s, FvGeo g, const double* vGrad, double ck, double ce, double delta, double* nut);
// alphaf.a[0] == nullptr: alphacf is re-formed from alpha (no face array kept)
int launch_assemble_momentum(hipStream_t s, FvGeo g, const double* U, const double* Uold, const double* alpha, const double* alphaOld,
                             CFace3 alphaf, CFace3 phi, const double* uSource, const double* uSourceDrag, const double* divG,
                             const double* vGrad /* grad(U) of the current iterate: linearUpwind only */, Mom7 M, double* src, double* rAU,
                             const PorousDev* por /* porous zones (porous.hpp), or nullptr: none; needs M.bd */);
// Gauss-linear gradient of magSqr(U) (three per cell): what the NVD / TVD limited schemes' gradient ratio r is formed from (passed to
// launch_assemble_momentum in vGrad's place when g.upwind >= 3)
int launch_grad_magsqr(hipStream_t s, FvGeo g, const double* U, double* gradL);
int launch_interp_rAU(hipStream_t s, FvGeo g, const double* rAU, Face3 rAUf);
// rAUf = interpolate(rAU) and phiForces (UcEqn.H:15-20) as one cell-centred sweep
// adjustPhi (icoFoamYade.C:108, pEqn.H:13-16): partial sums {massIn, fixedMassOut, adjustableMassOut, sum |internal flux|}; apply scales the
// outflow of the patches that do not fix U (and refreshes snGrad(p) of fixedFluxPressure patches); *err = 1 where OpenFOAM would stop
int launch_adjust_phi_sums(hipStream_t s, FvGeo g, CFace3 phiHbyA, CFace3 phiForces, double* partials);
int launch_adjust_phi_apply(hipStream_t s, FvGeo g, const double* sums, Face3 phiHbyA, CFace3 phiForces, CFace3 rAUf, const double* U, Face3 psn, int* err);
int launch_rAUf_phi_forces(hipStream_t s, FvGeo g, const double* rAU, const double* uSource, Face3 rf, Face3 out);
int launch_bmom(hipStream_t s, FvGeo g, const double* src, const double* p, CFace3 psn, CFace3 phiForces, CFace3 rAUf, double* bmom);
// pimple: launch_rAUf_phi_forces + launch_bmom as one sweep (round 5); rAUf_out.a[0] == nullptr: rAUcf is not stored (nobody streams it)
int launch_bmom_faces(hipStream_t s, FvGeo g, const double* rAU, const double* uSource, const double* src, const double* p, CFace3 psn, Face3 rAUf_out,
                      Face3 phiForces, double* bmom);
// one fused Jacobi pass: residual sums of x (slots 0..2), norm-factor sums (slots 3..5, uses xbar[3]) and xn = next iterate
// HbyA != nullptr: the pass also writes HbyA = rAU H(x) / V of its iterate x (launch_HbyA's result for U = x: hsrc = the momentum source, rAU)
int launch_mom_pass(hipStream_t s, FvGeo g, Mom7 M, const double* b, const double* x, double* xn, const double* xsum /* [3] component sums of x (device) */,
                    double n_glob, double* partials, const double* hsrc = nullptr, const double* rAU = nullptr, double* HbyA = nullptr);
int launch_HbyA(hipStream_t s, FvGeo g, Mom7 M, const double* src, const double* U, const double* rAU, double* HbyA);
int launch_phiHbyA(hipStream_t s, FvGeo g, const double* HbyA, const double* U, const double* Uold, CFace3 phiOld, CFace3 rAUf,
                   CFace3 alphaf, CFace3 phiForces, Face3 phiHbyA, Face3 psn, Face3 ddtc = Face3{} /* scratch face field for the ddtCorr term */,
                   int keep = 0 /* 1: store the ddtCorr term in ddtc, 2: read it from there (later correctors of the same momentum assembly) */);
int launch_assemble_pressure(hipStream_t s, FvGeo g, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn, const double* alpha,
                             const double* alphaOld, PMat A, double* rhs, bool matrix = true /* false: the matrix of the previous corrector stands, right-hand side only */);
int launch_flux_correct(hipStream_t s, FvGeo g, const double* p, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn, CFace3 phiForces /* pimple */,
                        Face3 pflux /* ico: pEqn.flux(); pimple: (phicForces - pEqn.flux() / alphacf) / rAUcf, the face term k_U_correct sums */, Face3 phi);
int launch_cont_err(hipStream_t s, FvGeo g, CFace3 phi, CFace3 alphaf, const double* alpha, const double* alphaOld, double* partials);   // slots 0,1
int launch_U_correct(hipStream_t s, FvGeo g, const double* HbyA, const double* rAU, const double* p, CFace3 psn, CFace3 phiForces,
                     CFace3 pflux, CFace3 alphaf, CFace3 rAUf, double* U);
// the same sweep + continuity errors (slots 0, 1) + next step's Courant sums (slots 2 max, 3 sum) of `phi`
int launch_U_correct_diag(hipStream_t s, FvGeo g, const double* HbyA, const double* rAU, const double* p, CFace3 psn, CFace3 phiForces,
                          CFace3 pflux, CFace3 alphaf, CFace3 rAUf, double* U, CFace3 phi, const double* alpha, const double* alphaOld, double* partials);

// ---- fused corrector sweeps (round 5; fv_kernels.hip "fused corrector sweeps"): same per-face expressions as the kernels above, same bits
// flux correction + velocity correction in one sweep; partials != nullptr: also the continuity errors (slots 0, 1) and the next pass's Courant sums
// (slots 2 max, 3 sum).  faces_from_cells: rAUf / alphacf are re-formed from rAU / alpha (their linear interpolates) instead of streamed from the face arrays
int launch_corr_back(hipStream_t s, FvGeo g, const double* p, CFace3 phiHbyA, CFace3 rAUf, CFace3 alphaf, CFace3 psn, CFace3 phiForces, Face3 phi,
                     const double* HbyA, const double* rAU, double* U, const double* alpha, const double* alphaOld, double* partials, bool faces_from_cells);
// phiHbyA (+ constrainPressure) + pressure assembly + PCG's first residual res = rhs - A x with k_p_init's two sums (slots 0, 1) in one sweep;
// dcorr: the face field launch_pre_coupling left at the start of the step; store_A = false: the matrix of the previous corrector stands.  Not for
// cases where adjustPhi acts between phiHbyA and the assembly
int launch_corr_front(hipStream_t s, FvGeo g, const double* HbyA, const double* U, CFace3 dcorr, CFace3 rAUf, CFace3 alphaf, CFace3 phiForces, Face3 phiHbyA,
                      Face3 psn, const double* rAU, const double* alpha, const double* alphaOld, PMat A, double* rhs, bool store_A, const double* x,
                      const double* xsum_dev, double xsum_val, double inv_n, double* res, double* partials, bool faces_from_cells);


// slab interfaces: coefficient of the z-face below the first owned plane, stored at the ghost cell under it (what p_row reads as uz[c - sz])
int launch_p_ghost_uz(hipStream_t s, FvGeo g, CFace3 rAUf, CFace3 alphaf, PMat A);
// boundary values as the equations see them, per boundary face of a single-domain block (the six sides x- x+ y- y+ z- z+, each with the lower remaining axis
// fastest): pb [nb], ub [nb][3], tb [nb]; a null output is skipped
int launch_boundary_values(hipStream_t s, FvGeo g, const double* p, CFace3 psn, const double* U, const double* T, TPatch te, double* pb, double* ub, double* tb);
// fy::Monitors' face kernel (monitors.hpp): the five partials of every wanted component of every surface object, nblk blocks per object
int launch_monitor_faces(hipStream_t s, FvGeo g, MonFaceTable t, const double* p, CFace3 psn, const double* U, const double* T, TPatch te, CFace3 phi, double* partials, int nblk);
// fy::WallLoads' face kernel (wall_loads.hpp): every due object's per-face outputs and the partials of its components, nblk blocks per object
int launch_wall_loads(hipStream_t s, FvGeo g, WlTable t, WlBlockGeo wg, const double* p, CFace3 psn, const double* U, double* wss, double* yplus, double* partials, int nblk);
// "nut_boundary" / "nearWallDist" per boundary face in the order of launch_boundary_values; a null output is skipped
int launch_wall_readouts(hipStream_t s, FvGeo g, double* nutb, double* yw);
