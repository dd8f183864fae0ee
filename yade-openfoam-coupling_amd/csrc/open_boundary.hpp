// Open boundaries on the general mesh (DESIGN.md section 3 "Open boundaries"; DESIGN_FV.md "Open boundaries"): a patch where the flux may change sign face by face --
// U inletOutlet (FY_BC_U_INLET_OUTLET) and pressureInletOutletVelocity (FY_BC_U_PRESSURE_INLET_OUTLET), k / epsilon / T inletOutlet (FY_BC_NUT_INLET_OUTLET,
// FY_BC_T_INLET_OUTLET) [OF-6 inletOutletFvPatchField, pressureInletOutletVelocityFvPatchVectorField, as recalled: OpenFOAM is not at hand to pin them].
//
// The conditions SELECT, they never blend: the value fraction of a face is exactly 0 or 1, read from the inflow mask -- one byte per boundary face,
//     u_inflow[f - nInt] = phi[f] < 0        on the faces of the patches that carry an open code for U, k, epsilon or T;  0 elsewhere
// (LduGeo::u_inflow; null: no open patch, nothing allocated, nothing launched).  The kernels of ldu_kernels.hip route a face through the code of the condition it
// equals: an inflow face is the patch's fixedValue face (pressureInletOutletVelocity: the transform-patch form, slip_face's), an outflow face a zeroGradient face.
//
// The mask is renewed by ONE kernel, k_ldu_open_faces, at three points:
//   (a) at the start of step(), before the first launch_ldu_grad_vec                                   [updateCoeffs() at matrix construction: the old time's flux]
//   (b) after each corrector's flux update (launch_ldu_flux_correct, launch_ldu_pim_flux) and before the velocity is corrected or reconstructed
//                                                                                                      [evaluate() in correctBoundaryConditions(): the new flux]
//   (c) after createPhi at create, at set_inlets and at fy_ldu_solver_write_field_host("U"): those form phi with every open face evaluated as zeroGradient first
// The same launch leaves the block partials of three sums over the open faces -- the number of inflow faces, the sum of phi over them, the sum of phi over the outflow
// faces -- which the shared fold (launch_reduce_finalize) adds in a fixed order: the same bits from run to run, and no host synchronisation in the step.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldu.hpp"

namespace fy {

enum { OPEN_INFLOW_FACES = 0, OPEN_INFLOW_FLUX, OPEN_OUTFLOW_FLUX, OPEN_SUMS };

// mask[b] = open[patch_of[b]] && phi[nInt + b] < 0 for the nb = nFaces - nInt boundary faces; partials: OPEN_SUMS slots in launch_reduce_finalize's layout for nb
int launch_ldu_open_faces(hipStream_t s, LduGeo g, const int32_t* open_patch, const double* phi, uint8_t* mask, double* partials);
// out[b] = mask[b] as a double (the "U_open_inflow" read-out)
int launch_ldu_open_mask_f64(hipStream_t s, int nb, const uint8_t* mask, double* out);

}  // namespace fy
