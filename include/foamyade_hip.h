/* foamyade_hip.h -- C-ABI of libfoamyade_hip.so: the MI355X-native drop-in for the hot path of
 * dpkn31/Yade-OpenFOAM-coupling (class Foam::FoamYade + the icoFoamYade / pimpleFoamYade loop bodies).
 *
 * Plain C: pointers and sizes only, no C++/torch types, int status codes, never throws.
 * Every entry point names the reference interface it replaces (paths relative to /root/reference).
 *
 * Two objects:
 *   fy_ctx     <->  Foam::FoamYade            FoamYade/FoamYade.H:57-161   (coupling engine, particle half)
 *   fy_solver  <->  the solver executables    icoFoamYade/icoFoamYade.C:38-154, pimpleFoamYade/pimpleFoamYade.C:40-119
 *                                             (+UcEqn.H, pEqn.H, CourantNo.H, continuityErrs.H, createFields.H)
 *
 * Memory layout at the boundary is OpenFOAM's: scalar = double, label = int, vector = 3 contiguous doubles
 * (xyzxyz...), tensor = 9 contiguous doubles row-major xx xy xz yx yy yz zx zy zz (FoamYade.C:450,472-474).
 * Particle records are the wire layout: 10 doubles [x y z vx vy vz wx wy wz radius] (FoamYade.C:190-219);
 * force records 6 doubles [Fx Fy Fz Tx Ty Tz] (FoamYade.C:492-498).
 */
#ifndef FOAMYADE_HIP_H
#define FOAMYADE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FY_ABI_VERSION 28

/* ---- status codes ------------------------------------------------------------------------------------ */
enum {
    FY_OK = 0,
    FY_ERR_INVALID = 1,     /* bad argument / call order */
    FY_ERR_NO_DEVICE = 2,   /* no gfx950 device visible: the product NEVER falls back to a CPU path */
    FY_ERR_HIP = 3,         /* a HIP runtime call failed; see fy_last_error() */
    FY_ERR_TRANSPORT = 4,   /* a transport callback returned non-zero */
    FY_ERR_UNSUPPORTED = 5,
    FY_ERR_NOT_CONVERGED = 6
};
const char* fy_last_error(void);      /* thread-local text of the last failure */
int fy_abi_version(void);
int fy_device_count(void);            /* number of visible HIP devices (0 on a CPU-only host) */

/* ---- where a caller-owned array lives ------------------------------------------------------------------ */
enum { FY_MEM_HOST = 0, FY_MEM_DEVICE = 1 };

/* ---- mesh: what FoamYade reads from fvMesh (mesh.C(), mesh.V(), mesh.points(); FoamYade.H:121, FoamYade.C:69,86,304) */
typedef struct fy_mesh_desc {
    int32_t n_cells;
    const double* centres;      /* [n_cells][3]  mesh.C(), HOST memory (read once at create) */
    const double* volumes;      /* [n_cells]     mesh.V(), HOST memory */
    double bbox_min[3];         /* bounding box of mesh.points() (FoamYade.C:82-94) */
    double bbox_max[3];
    /* Uniform hex block in blockMesh order (cell = i + nx*(j + ny*k)).  Required for point-force mode, where it
     * stands in for polyMesh::findCell (FoamYade.C:251), and for fy_solver.  Set nx = 0 for "unstructured". */
    int32_t nx, ny, nz;
    double dx;
    double origin[3];
    /* A GRADED (rectilinear) block in the same cell order: coordinates of the nx + 1, ny + 1, nz + 1 face planes along the axes (HOST memory,
     * copied at create); all NULL = the uniform block above.  With them findCell is a search along each axis, the k-d tree carries explicit
     * node coordinates (the centres as given) and dx is unused. */
    const double *xf, *yf, *zf;
} fy_mesh_desc;

/* ---- the twelve constructor arguments of Foam::FoamYade (FoamYade.H:106-117), minus mesh and the bool ---- */
typedef struct fy_field_ptrs {
    int32_t location;           /* FY_MEM_HOST: staged over PCIe each step; FY_MEM_DEVICE: used in place */
    const double* U;            /* [n][3] */
    const double* gradP;        /* [n][3] */
    const double* vGrad;        /* [n][9] */
    const double* divT;         /* [n][3] */
    const double* ddtU;         /* [n][3]  (only consumer is addedMassForce, FoamYade.C:392-413: see fy_set_force_models) */
    double g[3];                /* uniformDimensionedVectorField g */
    double* uSourceDrag;        /* [n]     read-write */
    double* alpha;              /* [n]     read-write */
    double* uSource;            /* [n][3]  read-write */
    double* uParticle;          /* [n][3]  read-write */
} fy_field_ptrs;

/* ---- transport: the MPI calls FoamYade.C makes, as callbacks, so that this library does not link an MPI -- */
/* datatype / op selectors for the callbacks */
enum { FY_T_INT = 0, FY_T_DOUBLE = 1 };
enum { FY_OP_MAX = 0, FY_OP_SUM = 1 };
/* All callbacks return 0 on success.  "world" = MPI_COMM_WORLD (Yade ranks first, README.md:29, FoamYade.C:28-43),
 * "local" = PstreamGlobals::MPI_COMM_FOAM (FoamYade.C:21-22). */
struct fy_wire_pieces;
typedef struct fy_transport {
    void* user;
    int32_t world_rank, world_size;     /* FoamYade.C:24-25 */
    int32_t local_rank, local_size;     /* FoamYade.C:21-22 */
    int (*send)(void* user, const void* buf, int count, int dtype, int dest, int tag);              /* MPI_Send / Isend+Wait */
    int (*recv)(void* user, void* buf, int count, int dtype, int src, int tag);                     /* MPI_Recv */
    int (*bcast_world)(void* user, void* buf, int count, int dtype, int root);                      /* MPI_Bcast(WORLD) */
    int (*bcast_local)(void* user, void* buf, int count, int dtype, int root);                      /* MPI_Bcast(MPI_COMM_FOAM) */
    int (*allreduce_world)(void* user, const void* in, void* out, int count, int dtype, int op);    /* MPI_Allreduce(WORLD) */
    /* ---- optional zero-copy wire (round 4; every pointer may be NULL: a zero-initialised struct is the round-3 transport) ----
     * A transport that owns staging memory -- the shared-memory arena that wire-helper ranks fill in parallel (include/foamyade_mpi.h:
     * one receiving core copies ~9 GB/s out of the MPI library whatever it posts, so the 800 MB of a 10 M-particle step need SEVERAL
     * receiving processes; measured: tools/native/mpi_recv_rate.cpp) -- hands the library VIEWS of the messages instead of copying them
     * into buffers of the library: the PCIe copies then start from / end in that memory.  Parallel-Yade protocol only. */
    /* called once from fy_create, before the bounding box goes out (FoamYade.C:77-111): the uniform block this rank computes on */
    int (*describe_block)(void* user, const double origin[3], double dx, const int32_t n[3]);
    /* recv(..., src, FY_TAG 1002) without the copy: *buf = the message where the transport keeps it (valid until the step's last send_commit).
     * The message may be the concatenation of several PIECES, each received by another helper for its own cell layers [k0, k1) across one axis: a record is
     * located only within its piece's layers (a particle near a cut arrives in both pieces and is found in exactly one). */
    int (*recv_view)(void* user, const void** buf, int count, int dtype, int src, int tag, struct fy_wire_pieces* pieces);
    /* the same in two halves (both or neither): recv_view_layout returns at once -- where the message WILL lie and how it is cut -- and
     * recv_view_next blocks until one more piece of this step's messages has landed and says which (src = the worker, piece = index into that
     * message's fy_wire_pieces; a message without cuts is its own piece 0).  The library then starts each piece's PCIe copy when it lands, in
     * whatever order the workers deliver, instead of each message's when it is complete. */
    int (*recv_view_layout)(void* user, const void** buf, int count, int dtype, int src, int tag, struct fy_wire_pieces* pieces);
    int (*recv_view_next)(void* user, int* src, int* piece);
    /* where the library should write a message it is about to send (count elements), then the hand-over: replaces send(...) */
    int (*send_reserve)(void* user, void** buf, int count, int dtype, int dest, int tag);
    int (*send_commit)(void* user, const void* buf, int count, int dtype, int dest, int tag);
    /* the memory the views point into, for page-locking (hipHostRegister) while `generation` stays the same; bytes = 0: nothing to lock */
    int (*view_region)(void* user, void** base, size_t* bytes, uint64_t* generation);
} fy_transport;
#define FY_WIRE_MAX_PIECES 8
typedef struct fy_wire_pieces {
    int32_t n;                                  /* 0: one message, no cuts */
    int32_t axis;                               /* the block is cut across this axis (0 x, 1 y, 2 z) */
    int32_t start[FY_WIRE_MAX_PIECES];          /* first record of piece q within the message */
    int32_t k0[FY_WIRE_MAX_PIECES], k1[FY_WIRE_MAX_PIECES];      /* cell layers [k0, k1) along `axis` piece q's records may be located in */
} fy_wire_pieces;

typedef struct fy_ctx fy_ctx;

/* Foam::FoamYade::FoamYade(...) FoamYade.H:106-122 -> getRankSize() FoamYade.C:18-53:
 * rank discovery, k-d tree build over mesh.C() (meshTree.C:9-37), bbox send to every Yade rank in parallel-Yade
 * mode (FoamYade.C:77-111), initFields (FoamYade.C:56-73).
 * transport == NULL selects "direct" mode: no wire traffic; particles are handed over with
 * fy_set_particles_* and forces read back with fy_get_forces_* (used by fy_solver, the tests and bench.py). */
int fy_create(const fy_mesh_desc* mesh, const fy_field_ptrs* fields, int gaussian_interp,
              const fy_transport* transport, int device_ordinal, fy_ctx** out);
/* FoamYade::setScalarProperties FoamYade.C:9-11 */
int fy_set_scalar_properties(fy_ctx*, double rhoP, double rhoF, double nu);
/* The two Gaussian-mode force models FoamYade carries WITHOUT a live call site; both are off by default, which is the shipped
 * behaviour.  Enabling one is what re-enabling it in the reference would do:
 *   FY_FORCE_GAUSSIAN_TORQUE  calcHydroTorque's Gaussian branch, FoamYade.C:465-479 (its call is commented out at FoamYade.C:618);
 *                             reads fields.vGrad and the angular velocity of the records; fills force[3..5]
 *   FY_FORCE_ADDED_MASS       addedMassForce, FoamYade.C:392-413 (never called): reads fields.ddtU and the dt passed to
 *                             fy_set_particle_action; adds to force[0..2] and back-scatters into uSource
 * A third flag is a model the reference does not have at all:
 *   FY_FORCE_SAFFMAN_MEI_LIFT Saffman's shear lift with Mei's finite-Reynolds-number factor on the interpolated vorticity w = curl U (reads fields.vGrad):
 *                             Re_p = |u_r| d / nu, Re_w = |w| d^2 / nu, b = Re_w / (2 (Re_p + small)), a = 0.3314 sqrt(b),
 *                             f = Re_p < 40 ? (1 - a) exp(-Re_p / 10) + a : 0.0524 sqrt(b Re_p), Cl = 3 / (2 pi sqrt(Re_w + small)) 6.46 f,
 *                             F = rho_f pv Cl (u_r x w); adds to force[0..2] and back-scatters into uSource like Archimedes' force
 * Returns FY_ERR_INVALID in point-force mode or when the field a model needs was not supplied to fy_create. */
#define FY_FORCE_ADDED_MASS 1u
#define FY_FORCE_GAUSSIAN_TORQUE 2u
#define FY_FORCE_SAFFMAN_MEI_LIFT 4u
int fy_set_force_models(fy_ctx*, unsigned flags);
/* The drag closure.  FY_DRAG_REFERENCE (the default) is what FoamYade computes: Wen-Yu / Ergun switched at alpha_f = 0.8 in Gaussian mode
 * (FoamYade.C:366-382), Stokes drag in point-force mode (FoamYade.C:437-444).  The others replace it; with eps = alpha_f, phi = max(1 - eps, 0),
 * m = |u_r| and Re = small + m d / nu they give K = beta / phi, the force pv K u_r and the scattered coefficient K phi (formulas: DESIGN.md section 3):
 *   Gaussian mode    FY_DRAG_DI_FELICE, FY_DRAG_KOCH_HILL, FY_DRAG_BEETSTRA
 *   point-force mode FY_DRAG_SCHILLER_NAUMANN: Stokes drag times f = Re < 1000 ? 1 + 0.15 Re^0.687 : 0.44 Re / 24
 * One law for all particles.  Returns FY_ERR_INVALID (the message lists the names the mode accepts) for a law of the other mode or an unknown value. */
#define FY_DRAG_REFERENCE 0
#define FY_DRAG_DI_FELICE 1
#define FY_DRAG_KOCH_HILL 2
#define FY_DRAG_BEETSTRA 3
#define FY_DRAG_SCHILLER_NAUMANN 4
int fy_set_drag_law(fy_ctx*, int law);
/* FoamYade::fibreCpl (public flag, FoamYade.H:102; off by default and never set by the two solvers).  When on, Yade sends 15 doubles per
 * particle instead of 10 (FoamYade.C:131-136 parallel, :161-165 serial) and the position is read with that stride (:194-198) while
 * velocity, spin and radius are still read from buf[np*10+3..9] of the same buffer (:211-221) -- mirrored literally.  After this call
 * fy_set_particles_host/_device take [n][15] records and the transport receives 15 n doubles.  Not available with z-slabs. */
int fy_set_fibre_coupling(fy_ctx*, int on);
/* FoamYade::setParticleAction FoamYade.C:605-632 (blocking).  On return alpha, uParticle, uSourceDrag, uSource hold
 * this step's values and (with a transport) found flags / forces / dt have been exchanged with Yade. */
int fy_set_particle_action(fy_ctx*, double dt);
/* FoamYade::setSourceZero FoamYade.C:556-566 */
int fy_set_source_zero(fy_ctx*);
/* FoamYade::finalizeRun (FoamYade.C:595-599; declared FoamYade.H:159, never called by the two solvers): the value Yade's rank 0 broadcasts over
   the world communicator; 10 means "finalize MPI now" -- which the caller does, the library does not own the MPI session */
int fy_finalize_run(fy_ctx*, int* value_out);
/* FoamYade::~FoamYade FoamYade.H:160 */
int fy_destroy(fy_ctx*);

/* ---- direct mode (no Yade peer): one call per "Yade proc" batch, batches are processed in index order exactly
 *      like the loop over inCommProcs (FoamYade.C:612-628) ------------------------------------------------- */
int fy_set_num_batches(fy_ctx*, int nbatch);
int fy_set_particles_host(fy_ctx*, int batch, const double* records, int64_t n);     /* copies (H2D); `records` may be reused or freed on return */
int fy_set_particles_device(fy_ctx*, int batch, const double* d_records, int64_t n); /* borrows the device pointer */
int fy_get_forces_host(fy_ctx*, int batch, double* out_forces /* [n][6] */);
/* z-slab mode (fy_solver_create_slab): hand the particles of batch 0 whose containing cell now lies in a neighbour's planes to that
 * neighbour over the slab communicator (ncclSend / ncclRecv in one group under RCCL -- the path the halos take), compact the rest.  A
 * particle moves at most one slab per call.  d_tags (device, optional): one int64 per record, e.g. the DEM's particle id; it travels with
 * the record and is rewritten in the new local order (tag_capacity entries available).  Afterwards the records are library-owned
 * (fy_get_particles_host reads them back).  Collective.  Single domain: a no-op. */
int fy_migrate_particles(fy_ctx*, int64_t* d_tags, int64_t tag_capacity, int64_t* n_local_out);
int fy_get_particles_host(fy_ctx*, int batch, double* records_out /* [n][10] or NULL */, int64_t* n_out);
int fy_get_found_host(fy_ctx*, int batch, int32_t* out_found /* [n], 1 / -1 as foundBuff FoamYade.C:141,222 */);
const double* fy_forces_device(fy_ctx*, int batch);
/* per-particle stencil of the last step, for parity tests: k[n], ids[n][16] (-1 padded, ascending d2, ids[0] =
 * inCell FoamYade.C:208), weights[n][16] (FoamYade.C:293-316), chain_len[n] (>12 => reference behaviour is undefined,
 * meshTree.H:66-68; we append and never evict) */
int fy_get_stencils_host(fy_ctx*, int batch, int32_t* k, int32_t* ids, double* weights, int32_t* chain_len);
/* k-d tree in preorder (node, left subtree, right subtree): cell ids, for parity with meshTree.C:19-37 */
int fy_get_tree_preorder(fy_ctx*, int32_t* out_ids /* [n_cells] */);
/* meshTree::nearestCell (meshTree.C:66-135) for n points, pos[n][3] on the host: out[q] = id of the nearest cell centre (among equidistant
   ones the first the reference's depth-first descent meets).  FoamYade itself never calls it (its Gaussian locate is the range search, its
   point locate mesh.findCell); exposed because it is the tree's public API and the findCell stand-in on general meshes. */
int fy_nearest_cells_host(fy_ctx*, const double* pos, int64_t n, int32_t* out);
/* read / write any of the ctx's cell fields by name ("alpha","uParticle","uSourceDrag","uSource","U","gradP","vGrad","divT") */
int fy_read_field_host(fy_ctx*, const char* name, double* out);
int fy_write_field_host(fy_ctx*, const char* name, const double* in);
double fy_yade_dt(fy_ctx*);           /* yadeDT received in exchangeDT (FoamYade.C:537-553) */
double fy_interp_range(fy_ctx*);      /* interpRange = 4*cbrt(V[0]) (FoamYade.C:69) */
/* Gaussian locate on a uniform block: how many particles of the last fy_set_particle_action were NOT placed through the per-(cell,
 * octant) candidate lists and took the plain tree walk instead (within 8e-6 dx of a cell face, outside the block, list overflow);
 * -1 when the lists are not in use (explicit tree, FOAMYADE_NO_LOCATE_LISTS, no memory).  Same results either way. */
long long fy_locate_walk_count(fy_ctx*);
/* Gaussian locate on an explicit tree (graded block, general mesh): entries per lane of the LDS stack the last step's walk ran with -- chosen from the kernel's own histogram of
 * the depths the walks need; a walk that needs more takes a second launch with the full depth --, 0 while the walk still runs with the full depth (first steps, small clouds),
 * -1 when the tree is not explicit.  Same results either way. */
int fy_locate_stack_depth(fy_ctx*);

/* per-phase device timings of the last fy_set_particle_action, milliseconds (HIP events on the ctx stream) */
typedef struct fy_particle_timings {
    double h2d, bin, locate_deposit, finalize, force, d2h, total;
    int64_t n_particles, n_pairs;     /* n_pairs = sum of k */
    /* drop-in path (a transport is attached; all 0 otherwise).  h2d / d2h above then hold the whole receive / send phases as the
       compute stream saw them; the four below split them: time on the PCIe copy stream and host time inside the transport calls */
    double copy_in, copy_out;         /* first H2D start .. last H2D end, first D2H start .. last D2H end (copy stream, ms) */
    double wire_recv, wire_send;      /* host wall time in the transport's record / result calls (ms) */
    int64_t bytes_in, bytes_out;      /* bytes that crossed PCIe in each direction (records; forces + found flags) */
    /* Gaussian mode: locate_deposit and force above are the two big kernels ALONE (k_locate_deposit; k_force_gaussian), bracketed by HIP
       events on their stream; finalize = cell-record pack + tile reduce + k_finalize_cells (+ slab halos); fold = tile reduce +
       k_fold_sources (+ slab halos) */
    double fold;
} fy_particle_timings;
int fy_get_particle_timings(fy_ctx*, fy_particle_timings* out);
int fy_enable_timing(fy_ctx*, int on);

/* ======================================================================================================== */
/* fy_solver: the time-loop bodies of icoFoamYade (PISO, point force) and pimpleFoamYade (PIMPLE, 4-way).  */
/* ======================================================================================================== */
enum { FY_SOLVER_ICO = 0, FY_SOLVER_PIMPLE = 1 };
/* boundary patches of the block, in this order */
enum { FY_XMIN = 0, FY_XMAX = 1, FY_YMIN = 2, FY_YMAX = 3, FY_ZMIN = 4, FY_ZMAX = 5 };
enum { FY_BC_U_FIXED_VALUE = 0, FY_BC_U_ZERO_GRADIENT = 1,
       FY_BC_U_SLIP = 2 /* symmetryPlane / symmetry / slip on the block's (planar) side: normal component 0, tangential components zeroGradient */,
       /* open boundaries, fy_ldu_solver only (fy_solver_create refuses them as unknown); see "Open boundaries" at fy_ldu_solver_get_open_boundary_stats */
       FY_BC_U_INLET_OUTLET = 3 /* inletOutlet: u_value where the flux enters (phi < 0), zeroGradient where it leaves */,
       FY_BC_U_PRESSURE_INLET_OUTLET = 4 /* pressureInletOutletVelocity: n (n . U_P) where the flux enters, zeroGradient where it leaves; takes no value */ };
enum { FY_BC_P_ZERO_GRADIENT = 0, FY_BC_P_FIXED_VALUE = 1, FY_BC_P_FIXED_FLUX = 2 };
enum { FY_PSOLVER_PCG_JACOBI = 0, FY_PSOLVER_PCG_MG = 1 };

#define FY_CONVECTION_LINEAR 0
#define FY_CONVECTION_UPWIND 1
#define FY_CONVECTION_LINEAR_UPWIND 2
/* NVD / TVD limited schemes [OF-6 LimitedScheme, NVDTVD]: face value = w U_owner + (1 - w) U_neighbour, w = limiter(r) w_linear + (1 - limiter(r)) pos0(flux),
   r = 2 (d . grad(magSqr(U))_upwind) / (magSqr(U)_N - magSqr(U)_P) - 1; one limiter for the three components, weights implicit */
#define FY_CONVECTION_LIMITED_LINEAR 3   /* Gauss limitedLinear k: max(min(2 r / k, 1), 0), k = convection_limiter_k in [0, 1] */
#define FY_CONVECTION_VAN_LEER 4         /* (r + |r|) / (1 + |r|) */
#define FY_CONVECTION_MUSCL 5            /* max(min(2 r, r / 2 + 1 / 2, 2), 0) */
#define FY_CONVECTION_MINMOD 6           /* max(min(r, 1), 0) */
#define FY_CONVECTION_SUPERBEE 7         /* max(min(2 r, 1), min(r, 2), 0) */
#define FY_CONVECTION_QUICK 8            /* max(min(2 r, (3 + r) / 4, 2), 0) */
/* continuousPhaseTurbulence (pimpleFoamYade/createFields.H, DPMTurbulenceModels.C:67-77; icoFoamYade has no turbulence model) */
#define FY_TURBULENCE_LAMINAR 0        /* simulationType laminar / laminarModel Stokes (DPMTurbulenceModels.C:67-68) */
#define FY_TURBULENCE_SMAGORINSKY 1    /* simulationType LES, LESModel Smagorinsky (DPMTurbulenceModels.C:73-74), delta cubeRootVol */
#define FY_TURBULENCE_KEQN 2           /* simulationType LES, LESModel kEqn (DPMTurbulenceModels.C:76-77), delta cubeRootVol */
#define FY_TURBULENCE_KEPSILON 3       /* simulationType RAS, RASModel kEpsilon (DPMTurbulenceModels.C:70-71) */
#define FY_BC_NUT_ZERO_GRADIENT 0
#define FY_BC_NUT_FIXED_VALUE 1
#define FY_BC_NUT_CALCULATED 3          /* nut_bc: `calculated` patch = the model's expression on the boundary values of k (and epsilon); kEqn / kEpsilon */
#define FY_BC_NUT_INLET_OUTLET 4        /* k_bc, eps_bc of fy_ldu_case only (nut_bc refuses it): inletOutlet -- the patch's value where the flux enters, zeroGradient where it leaves */
#define FY_BC_WALL_FUNCTION 2           /* nut_bc: nutkWallFunction (needs a model with k); eps_bc: epsilonWallFunction; k takes zeroGradient (kqRWallFunction) */
/* fieldAverage: running means and second central moments of cell fields, updated on the device once per step (OpenFOAM's fieldAverage function object
   [OF-6 fieldAverage, fieldAverageTemplates.C, as recalled: OpenFOAM is not at hand to pin it]).  An item is one field with its mean m and, with
   prime2_mean, P = prime2Mean: one value per cell for a scalar, six for a vector in symmTensor order xx xy xz yy yz zz.  Per item N samples and T seconds
   averaged; after a step of dt
       base time:      Dt = T + dt, a = (Dt - dt) / Dt, b = dt / Dt          base iteration: Dt = N + 1, a = (Dt - 1) / Dt, b = 1 / Dt
       per cell:       P = P + m m;  m_new = a m + b x;  P = (a P + b (x x)) - m_new m_new;  m = m_new;          then N += 1, T += dt
   The sample is taken at the end of the step where runTime.write() stands (icoFoamYade.C:142, pimpleFoamYade.C:107): before setSourceZero, so it sees the
   step's alpha / uSource / uParticle, with or without fy_solver_hold_sources.  (OpenFOAM executes function objects inside the next runTime.run(), after
   setSourceZero, where alpha is 1 everywhere: a deliberate difference)  A sample is taken only while elapsed >= start_after - dt / 2 and,
   with stop_after > 0, elapsed <= stop_after + dt / 2, elapsed being the sum of the steps' deltaT since the solver was created [OF-6 timeControl]. */
#define FY_AVERAGE_MAX_ITEMS 8
typedef struct fy_average_item {
    char field[32];                 /* solver field name: U, p, alpha, uParticle, uSource, nut, k, epsilon, T and the solid statistics' six fields -- where the solver has the field */
    int32_t prime2_mean;            /* also keep P */
    int32_t iteration_base;         /* 0: base time (weights deltaT), 1: base iteration (equal weights) */
} fy_average_item;
typedef struct fy_average_desc {
    int32_t n_items;                /* 0: no averaging -- no kernel, no memory, no file */
    fy_average_item items[FY_AVERAGE_MAX_ITEMS];
    double start_after, stop_after; /* the window in seconds since the solver was created; stop_after 0: no end */
} fy_average_desc;

/* Run-time monitors: OpenFOAM's volFieldValue / surfaceFieldValue function objects as reductions on the device ([OF-6 fieldValue, volFieldValue.C, surfaceFieldValue.C]
   as recalled: OpenFOAM is not at hand to pin them).  An object reduces up to 8 fields over all cells (FY_MONITOR_VOL) or over the boundary faces of
   one patch (FY_MONITOR_SURFACE), once every `interval` steps, where fieldAverage samples: after the last corrector, the turbulence correction and the T equation, before
   setSourceZero.  x_i = the field in cell i, or its boundary value on face i ("p_boundary" ... below; phi: the flux OUT of the domain); V_i the cell volume, A_i = |Sf_i|;
   w_i the weight field (volume: alpha; surface: phi, outward); n the number of cells / faces.  A vector field yields three values, component by component (min and max too).
       sum          sum_i x_i                               average            (sum_i x_i) / n                        min, max     over i
       volIntegrate sum_i x_i V_i                           volAverage         (sum_i x_i V_i) / (sum_i V_i)           weightedVolAverage  (sum_i (w_i V_i) x_i) / (sum_i w_i V_i)
       areaIntegrate sum_i x_i A_i                          areaAverage        (sum_i x_i A_i) / (sum_i A_i)           weightedAverage     (sum_i w_i x_i) / (sum_i w_i)
   Every sum is formed as per-256-block partials folded in a fixed order: FP64, no atomics, the same bits from run to run.  Each sample is one row {time, values} in a
   ring on the device; the host copies rows out only when the ring is full or when fy_solver_get_monitor_rows asks, so that sampling never waits for the device.
   time = start_time + the sum of the steps' deltaT since the solver was created. */
#define FY_MONITOR_MAX_OBJECTS 8
#define FY_MONITOR_MAX_FIELDS 8
#define FY_MONITOR_VOL 1
#define FY_MONITOR_SURFACE 2
enum { FY_MONITOR_SUM = 1, FY_MONITOR_AVERAGE, FY_MONITOR_VOL_AVERAGE, FY_MONITOR_VOL_INTEGRATE, FY_MONITOR_WEIGHTED_VOL_AVERAGE, FY_MONITOR_MIN, FY_MONITOR_MAX,
       FY_MONITOR_AREA_AVERAGE, FY_MONITOR_AREA_INTEGRATE, FY_MONITOR_WEIGHTED_AVERAGE };
typedef struct fy_monitor_object {
    char name[32];
    int32_t kind;                   /* FY_MONITOR_VOL | FY_MONITOR_SURFACE */
    int32_t patch;                  /* surface, fy_ldu_solver: the patch index; fy_solver: a mask of sides, bit 2 d + s (x- x+ y- y+ z- z+) -- one patch may cover several */
    int32_t operation;              /* FY_MONITOR_*: volume sum average volAverage volIntegrate weightedVolAverage min max; surface sum average areaAverage areaIntegrate weightedAverage min max */
    char weight_field[32];          /* weighted operations: "alpha" (volume) | "phi" (surface); else empty */
    int32_t interval;               /* one sample every `interval` steps, >= 1 (0 is read as 1) */
    int32_t n_fields;
    char fields[FY_MONITOR_MAX_FIELDS][32];      /* volume: what fieldAverage accepts on this solver; surface: phi, p, U, T */
} fy_monitor_object;
typedef struct fy_monitor_desc {
    int32_t n_objects;              /* 0: no monitors -- no kernel, no memory */
    fy_monitor_object objects[FY_MONITOR_MAX_OBJECTS];
    int32_t ring_rows;              /* rows of the device ring per object (0: 256) */
    double start_time;              /* the time of the solver's creation (a case's startTime) */
} fy_monitor_desc;

/* Wall loads: OpenFOAM's forces / wallShearStress / yPlus function objects on the device ([OF-6 forces.C, wallShearStress.C, yPlus.C] as recalled: unpinned, DESIGN.md
   sections 3 "Wall loads" and 5).  Sampled where the monitors are.  For a boundary face f of a selected patch, outward Sf, n = Sf / |Sf|, owner cell P:
       G_P[i][j] = d_i U_j      the Gauss-linear gradient of U in P (internal faces linearly interpolated, boundary faces their value as the equations see it)
       s = (U_b - U_P) delta    delta: the momentum equation's wall coefficient (1 / (n . (Cf - C_P)); half a cell on the block); 0 on a zeroGradient patch
       G_b = G_P + n (x) (s - n . G_P)          R_b = -nuEff_b dev(twoSymm(G_b)), nuEff_b = nu + nut_b (the void fraction does not enter)
       wallShearStress = -n . R_b               yPlus = Cmu^1/4 y sqrt(k_P) / nu on a nutkWallFunction patch, y sqrt(nuEff_b |s|) / nu elsewhere (y: nearWallDist)
       forces:  fP = rho Sf (p_b - p_ref)   fV = rho (Sf . R_b)   mP = (Cf - cofr) x fP   mV = (Cf - cofr) x fV, each summed over the object's faces
   Every bracket is one IEEE operation; the sums are per-256-block partials folded in a fixed order (no atomics, the same bits from run to run).  A forces row has 12
   values Fp_x Fp_y Fp_z Fv_x .. Mp_x .. Mv_z; a wallShearStress row per patch of its set min_x min_y min_z max_x max_y max_z; a yPlus row per patch min max average.
   Rows go to rings on the device as the monitors' do.  A patch set: fy_solver reads `sides` (a mask, bit 2 d + s), fy_ldu_solver patches[0 .. n_patches). */
#define FY_WALL_LOADS_MAX_FORCES 4
#define FY_WALL_LOADS_MAX_PATCHES 8
typedef struct fy_wall_patch_set {
    int32_t sides;                  /* fy_solver: mask of sides x- x+ y- y+ z- z+ */
    int32_t n_patches;              /* fy_ldu_solver: patch indices (no cyclic patch) */
    int32_t patches[FY_WALL_LOADS_MAX_PATCHES];
} fy_wall_patch_set;
typedef struct fy_forces_object {
    char name[32];
    fy_wall_patch_set set;
    double rho, p_ref, cofr[3];     /* rhoInf (> 0), pRef, CofR */
    int32_t interval;               /* one sample every `interval` steps, >= 1 (0 is read as 1) */
} fy_forces_object;
typedef struct fy_wall_field_object {
    int32_t on;
    fy_wall_patch_set set;
    int32_t interval;
} fy_wall_field_object;
typedef struct fy_wall_loads_desc {
    int32_t n_forces;               /* all zero (n_forces 0, both `on` 0): off -- no kernel, no memory */
    fy_forces_object forces[FY_WALL_LOADS_MAX_FORCES];
    fy_wall_field_object wall_shear_stress, y_plus;      /* objects "wallShearStress", "yPlus": per-face fields "wallShearStress_boundary" [nb][3], "yPlus_boundary" [nb] */
    int32_t ring_rows;              /* rows of the device ring per object (0: 256) */
    double start_time;
} fy_wall_loads_desc;

/* Inlets: a fixed-value velocity side (fy_solver) or patch (fy_ldu_solver) whose value varies over its faces and in time (DESIGN.md section 3 "Inlets").  Each face f
   of the side or patch carries
       U_f(t) = a_0(t) S_0,f + a_1(t) S_1,f + a_2(t) S_2,f                  (n_terms = 1 .. 3, summed left to right, every bracket one IEEE operation)
   a_m: a scalar function of time (fy_time_function), evaluated on the host in double once per step at the time the step advances to, start_time + the elapsed time of
   the steps so far + the step's own delta_t, right after that delta_t is fixed and before any kernel of the step reads a boundary value.  S_m: a vector shape --
   FY_SHAPE_UNIFORM one vector (shape[3]), FY_SHAPE_PER_FACE one per face (shape[n_faces][3], in the order in which "U_boundary" lists the side's or patch's faces), or
   FY_SHAPE_FLOW_RATE, which the library forms itself: -n_f / sum |S_f| over the side or patch (n_f the outward unit normal), so that a_m is the volumetric flow rate
   INTO the domain.  The side's or patch's u_value is then read nowhere.  One launch per step on the solver's stream (the "inlets" kernel clock), no host
   synchronisation, no atomics; the shapes are uploaded once.  phi is not touched: it picks up the new boundary flux where the loop re-forms it (OpenFOAM's fvc::grad(U)
   before UEqn would still see the previous value; here every consumer of the step sees the new one).
   Time functions restate OpenFOAM-6's Function1 set as recalled (unpinned):
       FY_TIME_CONSTANT   value
       FY_TIME_TABLE      linear interpolation of points[n_points][2] = (t, v), times strictly increasing; outside [t_0, t_last] FY_TIME_CLAMP holds the end value,
                          FY_TIME_REPEAT maps t to t_0 + (u - span floor(u / span)), u = t - t_0, span = t_last - t_0 (n_points >= 2 then)
       FY_TIME_SINE       amplitude sin(2 pi frequency (t - t0))
       FY_TIME_SQUARE     amplitude times +1 while frac(frequency (t - t0)) < mark_space / (1 + mark_space), else -1 (mark_space 0 is read as 1)
   All zero (n = 0): no inlets -- nothing allocated, nothing launched, and every kernel computes exactly what it did without them. */
#define FY_TIME_CONSTANT 0
#define FY_TIME_TABLE 1
#define FY_TIME_SINE 2
#define FY_TIME_SQUARE 3
#define FY_TIME_CLAMP 0
#define FY_TIME_REPEAT 1
#define FY_SHAPE_UNIFORM 0
#define FY_SHAPE_PER_FACE 1
#define FY_SHAPE_FLOW_RATE 2
#define FY_INLETS_MAX 16
typedef struct fy_time_function {
    int32_t kind;                   /* FY_TIME_* */
    double value;                   /* constant */
    double amplitude, frequency, t0, mark_space;      /* sine, square: frequency > 0 */
    int32_t n_points;               /* table */
    const double* points;           /* [n_points][2], copied when the inlets are set */
    int32_t out_of_bounds;          /* FY_TIME_CLAMP | FY_TIME_REPEAT */
} fy_time_function;
typedef struct fy_inlet_term {
    fy_time_function f;
    int32_t shape_kind;             /* FY_SHAPE_* */
    const double* shape;            /* [3] | [n_faces][3] | not read; copied when the inlets are set */
} fy_inlet_term;
typedef struct fy_inlet_desc {
    int32_t patch;                  /* fy_solver: the side 0 .. 5 (x- x+ y- y+ z- z+); fy_ldu_solver: the patch index.  It must be FY_BC_U_FIXED_VALUE */
    int32_t n_terms;                /* 1 .. 3 */
    fy_inlet_term terms[3];
} fy_inlet_desc;
typedef struct fy_inlets_desc {
    double start_time;
    int32_t n;                      /* 0 .. FY_INLETS_MAX, at most one inlet per side or patch */
    const fy_inlet_desc* inlets;
} fy_inlets_desc;
/* the value of a time function at t: the host arithmetic of the inlets, exported so that it can be checked without a device.  NaN for a NULL or malformed function */
double fy_time_function_eval(const fy_time_function* f, double t);

/* Fluid temperature with particle-fluid heat exchange (a capability the reference does not have; DESIGN.md section 3 "heat exchange", DESIGN_FV.md "T equation").
   Fluid: cp [J/kg/K], kappa [W/m/K], D = kappa / (rho_f cp), Pr = nu rho_f cp / kappa, Deff = D + nut / prt (nut = 0 when laminar).  A particle of diameter d and
   temperature Tp, with the force pass's stencil (cells c, normalised weights w; point-force mode: the containing cell, w = 1, eps = 1):
       eps = sum w alpha_c, u_f = sum w U_c, Re = small + |u_f - v_p| d / nu
       FY_NUSSELT_RANZ_MARSHALL   Nu = 2 + 0.6 Re^1/2 Pr^1/3                                                                  (both solvers)
       FY_NUSSELT_GUNN            Nu = (7 - 10 eps + 5 eps^2)(1 + 0.7 Res^0.2 Pr^1/3) + (1.33 - 2.4 eps + 1.2 eps^2) Res^0.7 Pr^1/3,  Res = eps Re     (pimpleFoamYade only)
       hA = Nu kappa pi d;  Sp_c += w hA,  Su_c += w hA Tp      [W/K, W]
   once per step, after the last corrector and the turbulence model's correct(), with the step's final flux F_f = alpha_f phi_f (outward) and alphaOld = alpha:
       alpha_c V_c (T - T_old) / dt + sum_f F_f T_f - T_c sum_f F_f - sum_f alpha_f Deff_f |S_f| / |d_f| (T_N - T_c) = (Su_c - Sp_c T_c) / (rho_f cp)
   (implicit; T_f linear | upwind; a Jacobi solve with T_tol / T_rel_tol / T_max_iter), and then q_p = hA (sum w T_c - Tp) [W into the particle]: sum_p q_p =
   sum_c (Sp_c T_c - Su_c) identically.  All zero: off -- nothing is allocated or launched.  Single domain only (fy_solver_create_slab refuses it), no fibre coupling. */
#define FY_NUSSELT_RANZ_MARSHALL 0
#define FY_NUSSELT_GUNN 1
#define FY_BC_T_ZERO_GRADIENT 0
#define FY_BC_T_FIXED_VALUE 1
#define FY_BC_T_INLET_OUTLET 2          /* fy_ldu_case.T_bc only: inletOutlet -- T_value where the flux enters, zeroGradient where it leaves */
typedef struct fy_thermal_desc {
    int32_t on;
    double cp, kappa;               /* > 0 */
    double prt;                     /* turbulent Prandtl number (> 0 with a turbulence model; 0: 1) */
    int32_t nusselt_law;            /* FY_NUSSELT_* */
    double T_initial;               /* uniform internalField of 0/T (fy_solver_write_field_host("T") for a non-uniform one) */
    int32_t T_bc[6]; double T_value[6];      /* FY_BC_T_* per side (fy_case_desc; not read on a general mesh: fy_ldu_case.T_bc / T_value per patch) */
    int32_t T_convection_scheme;    /* div(phi,T) / div(alphaPhic,T): FY_CONVECTION_LINEAR | FY_CONVECTION_UPWIND */
    double T_tol, T_rel_tol; int32_t T_max_iter;      /* solvers.T: not both tolerances zero, T_max_iter >= 1 */
    double particle_temperature;    /* Tp of every particle of a batch nobody gave temperatures (fy_solver_set_particle_temperatures_*) */
    /* The thermal loop (all three zero: off, the caller owns Tp and T is a passive scalar).
       particle_cp > 0 [J/kg/K; needs rho_particle > 0]: the library integrates Tp per particle, m_p c_pp dTp/dt = q_p with m_p = rho_particle (4/3) pi r^3, backward Euler
       for the particle-fluid pair: r_p = dt hA / (m_p c_pp), hA' = hA / (1 + r_p) takes hA's place in Sp / Su / q above and Tp += dt q / (m_p c_pp) after the T solve
       (dt: the step's own delta_t).  A particle nobody located keeps its Tp.
       beta [1/K], T_ref: Boussinesq buoyancy a_c = (-beta (T_c - T_ref)) g with the T the step found, added to uSource where the momentum equations read it (ico:
       the assembly; pimple: phicForces and the predictor's right-hand side, beside g); field "buoyancy" [n][3], kernel clock "buoyancy".  Off with beta == 0 or g == 0. */
    double particle_cp, beta, T_ref;
} fy_thermal_desc;

typedef struct fy_case_desc {
    int32_t solver;                 /* FY_SOLVER_ICO | FY_SOLVER_PIMPLE */
    int32_t nx, ny, nz;
    double dx;
    double origin[3];
    double dt;                      /* controlDict deltaT */
    double nu;                      /* transportProperties nu (icoFoamYade/createFields.H:29-33) */
    double rho_fluid, rho_particle; /* fluidDensity|rho.<phase>, partDensity */
    double g[3];                    /* constant/g */
    int32_t u_bc[6];  double u_value[6][3];
    int32_t p_bc[6];  double p_value[6];
    /* fvSolution PISO / PIMPLE dictionaries (icoFoamYade/createFields.H:166-169, pimpleFoamYade/createFields.H:83-86) */
    int32_t n_outer_correctors;     /* PIMPLE nOuterCorrectors (1 for PISO) */
    int32_t n_correctors;           /* nCorrectors */
    int32_t n_non_orth_correctors;  /* nNonOrthogonalCorrectors */
    int32_t momentum_predictor;
    int32_t p_ref_cell; double p_ref_value;
    /* linear solver controls: p, pFinal, U */
    int32_t p_solver;               /* FY_PSOLVER_* */
    double p_tol, p_rel_tol, p_final_tol, p_final_rel_tol; int32_t p_max_iter;
    double u_tol, u_rel_tol; int32_t u_max_iter;
    int32_t convection_scheme;             /* divSchemes for div(phi,U): FY_CONVECTION_LINEAR (Gauss linear, default) | _UPWIND (Gauss upwind) | _LINEAR_UPWIND (Gauss linearUpwind, unlimited) | the limited schemes _LIMITED_LINEAR .. _QUICK */
    /* controlDict adjustTimeStep / maxCo / maxDeltaT: readTimeControls.H + CourantNo.H + setDeltaT.H at the top of the time loop
       (pimpleFoamYade.C:62-64); dt above is then the initial deltaT and fy_step_stats.delta_t reports what each step used */
    int32_t adjust_time_step; double max_co, max_delta_t;
    /* fvSolution relaxationFactors: equations { Uc; UcFinal } for UcEqn.relax() (UcEqn.H:12), fields { p; pFinal } for p.relax()
       (pEqn.H:41).  <= 0: no entry (the call does nothing); the *_final values apply on the last outer corrector, falling back to the
       plain ones when absent.  fy_case_defaults: u_relax = 1 (the DPMFoam tutorials' `equations { ".*" 1; }`), no field relaxation */
    double u_relax, u_relax_final, p_relax, p_relax_final;
    /* constant/turbulenceProperties (pimpleFoamYade only): FY_TURBULENCE_*.  Smagorinsky [OF-6 Smagorinsky.C]: k from
       a = Ce/delta, b = 2/3 tr(D), c = 2 Ck delta (dev(D) && D), k = ((-b + sqrt(b^2 + 4ac)) / 2a)^2, nut = Ck delta sqrt(k), evaluated by
       continuousPhaseTurbulence->correct() after the last corrector of the final outer iteration (pimpleFoamYade.C:101-104);
       delta = les_delta_coeff * cbrt(V) (LESdelta cubeRootVol); nuEff = nu + nut enters divDevRhoReff (UcEqn.H:7) as
       -fvm::laplacian(alpha nuEff, U) - fvc::div(alpha nuEff dev2(T(grad U))).  nut_initial / nut_bc / nut_value: the 0/nut file */
    int32_t turbulence_model;
    double les_ck, les_ce, les_delta_coeff;      /* fy_case_defaults: 0.094, 1.048, 1 */
    int32_t nut_bc[6]; double nut_value[6];      /* FY_BC_NUT_* per side */
    double nut_initial;                          /* uniform internalField of 0/nut (fy_solver_write_field_host("nut") for a non-uniform one) */
    /* kEqn [OF-6 LES/kEqn/kEqn.C]: fvm::ddt(alpha,k) + fvm::div(alphaPhic,k) - fvm::laplacian(alpha (nut + nu), k) == alpha G
       - fvm::SuSp(2/3 alpha div(phic), k) - fvm::Sp(Ce alpha sqrt(k)/delta, k), G = nut (gradU && dev(twoSymm(gradU))); relax; solve; bound(k, kMin);
       nut = Ck sqrt(k) delta.  The 0/k file: k_initial (uniform), k_bc / k_value per side (FY_BC_NUT_* values: zeroGradient | fixedValue);
       divSchemes div(alphaPhic,k): k_convection_scheme FY_CONVECTION_LINEAR | _UPWIND; solvers.k: k_tol / k_rel_tol / k_max_iter;
       relaxationFactors equations k: k_relax (<= 0: none) */
    int32_t k_bc[6]; double k_value[6]; double k_initial;
    /* k_convection_scheme and eps_convection_scheme (below) -- fy_case_defaults: FY_CONVECTION_UPWIND; fy_ldu_case_defaults: FY_CONVECTION_LINEAR.
       THE TWO DEFAULTS DIFFER: a case that runs on both solvers, or is compared across them, names both schemes (on a side that carries a flux
       the two schemes put k 6e-3 of its maximum apart within one step) */
    int32_t k_convection_scheme;
    double k_tol, k_rel_tol; int32_t k_max_iter;
    double k_relax;
    /* kEpsilon [OF-6 RAS/kEpsilon/kEpsilon.C]: first the dissipation equation, fvm::ddt(alpha,eps) + fvm::div(alphaPhic,eps)
       - fvm::laplacian(alpha (nut/sigmaEps + nu), eps) == C1 alpha G eps/k - fvm::SuSp((2/3 C1 - C3) alpha div(phic), eps) - fvm::Sp(C2 alpha eps/k, eps),
       bound(eps, epsilonMin); then fvm::ddt(alpha,k) + fvm::div(alphaPhic,k) - fvm::laplacian(alpha (nut/sigmak + nu), k) == alpha G
       - fvm::SuSp(2/3 alpha div(phic), k) - fvm::Sp(alpha eps/k, k) with the NEW eps, bound(k, kMin); nut = Cmu k^2/eps.
       k uses the k_* fields above; epsilon its own.  Boundary types zeroGradient | fixedValue | FY_BC_WALL_FUNCTION (below) */
    double ras_cmu, ras_c1, ras_c2, ras_c3, ras_sigmak, ras_sigmaeps;   /* fy_case_defaults: 0.09, 1.44, 1.92, 0, 1, 1.3 */
    int32_t eps_bc[6]; double eps_value[6]; double eps_initial;
    int32_t eps_convection_scheme;               /* FY_CONVECTION_LINEAR | _UPWIND for div(alphaPhic,epsilon); default: see k_convection_scheme */
    double eps_tol, eps_rel_tol; int32_t eps_max_iter;
    double eps_relax;
    /* wall functions [OF-6 nutkWallFunction / epsilonWallFunction]: nut_w = nu (y+ kappa / ln(E y+) - 1) above yPlusLam, else 0, with
       y+ = Cmu^1/4 y sqrt(k)/nu; in the wall cells eps = Cmu^3/4 k^3/2/(kappa y) is imposed on the epsilon equation and the production G is
       replaced by (1/W) sum (nut_w + nu) |snGrad U| Cmu^1/4 sqrt(k)/(kappa y).  Cmu is ras_cmu */
    double wf_kappa, wf_E;                       /* fy_case_defaults: 0.41, 9.8 */
    /* A GRADED single block (blockMesh simpleGrading; icoFoamYade/createFields.H:15-162 and pimpleFoamYade/createFields.H:32-261 take any
       fvMesh): cell sizes along x, y, z -- nx, ny, nz doubles each, copied at fy_solver_create; all three NULL (fy_case_defaults) = uniform
       cubes of edge dx.  The block then starts at `origin`, dx is ignored.  Everything the uniform block carries except z-slabs (a graded
       block runs on one domain) */
    const double *hx, *hy, *hz;
    double convection_limiter_k;            /* FY_CONVECTION_LIMITED_LINEAR: the k of `Gauss limitedLinear k` (fy_case_defaults: 1) */
    /* constant/couplingProperties (optional; zero = the reference's behaviour): applied to the solver's coupling object at fy_solver_create with
       fy_set_drag_law / fy_set_force_models, whose refusals (a law of the other mode, models in point-force mode) then fail the create */
    int32_t drag_law;                       /* FY_DRAG_* */
    uint32_t force_models;                  /* FY_FORCE_* flags */
    /* controlDict functions: the fieldAverage object (all zero: none), applied at fy_solver_create with fy_solver_set_field_average */
    fy_average_desc average;
    /* constant/couplingProperties heatTransfer + 0/T: the fluid temperature equation and the particle-fluid heat exchange (all zero: off) */
    fy_thermal_desc thermal;
    /* controlDict functions: the volFieldValue / surfaceFieldValue objects (all zero: none), applied at fy_solver_create with fy_solver_set_monitors */
    fy_monitor_desc monitors;
    /* constant/couplingProperties solidStatistics: the solid-phase statistics, applied at fy_solver_create with fy_solver_set_solid_statistics (0: off) */
    int32_t solid_stats;
    /* inlets on fixed-value velocity sides (all zero: none -- nothing allocated, nothing launched), applied at fy_solver_create with fy_solver_set_inlets */
    fy_inlets_desc inlets;
    /* controlDict functions: the forces / wallShearStress / yPlus objects (all zero: none), applied at fy_solver_create with fy_solver_set_wall_loads */
    fy_wall_loads_desc wall_loads;
} fy_case_desc;

typedef struct fy_solver fy_solver;

typedef struct fy_step_stats {
    double courant_mean, courant_max;                   /* CourantNo.H:32-49 */
    double cont_err_sum_local, cont_err_global, cont_err_cumulative;   /* continuityErrs.H:32-46 */
    int32_t p_iters_total, p_solves, u_iters_total;
    double p_initial_residual, p_final_residual;
    double ms_particle, ms_momentum, ms_pressure, ms_other, ms_total;
    double delta_t;                                     /* the time step this pass used (setDeltaT.H when adjust_time_step) */
} fy_step_stats;

void fy_case_defaults(fy_case_desc* c, int solver);
int fy_solver_create(const fy_case_desc* c, const fy_transport* transport, int device_ordinal, fy_solver** out);
fy_ctx* fy_solver_coupling(fy_solver*);                 /* the yadeCoupling object (icoFoamYade.C:54, pimpleFoamYade.C:54) */
int fy_solver_step(fy_solver*);                         /* one pass of the while(runTime.loop()) body */
int fy_solver_get_stats(fy_solver*, fy_step_stats* out);
/* names: "U" [n][3], "p" [n], "phi_x" [(nx+1)*ny*nz], "phi_y", "phi_z", "nut" [n] (with a turbulence model), "k" [n] (kEqn, kEpsilon), "epsilon" [n] (kEpsilon), plus every fy_ctx field name.
   Diagnostics of the last step, for tests that hold the sweeps to a reference (the owned cells / faces): "rAU", "HbyA", "mom_diag", "mom_src", "p_diag", "p_ux", "p_uy",
   "p_uz", "p_rhs", "divG"; read-only: "mom_an0" .. "mom_an5" [n] (the momentum matrix's neighbour coefficient across side 2 d + s) and "phiHbyA_x" | "_y" | "_z" (face
   arrays like phi).  kEqn / kEpsilon and the T equation reuse the momentum matrix's storage: "HbyA", "mom_diag", "mom_an*" (and "mom_src" under a transport model) are
   FY_ERR_UNSUPPORTED there. */
int fy_solver_read_field_host(fy_solver*, const char* name, double* out);
int fy_solver_write_field_host(fy_solver*, const char* name, const double* in);
/* number of doubles fy_solver_read/write_field_host move for `name` on this rank (owned cells / local faces) */
int fy_solver_field_count(fy_solver*, const char* name, int64_t* count);
int fy_solver_destroy(fy_solver*);

/* By default fy_solver_step ends with yadeCoupling.setSourceZero() (icoFoamYade.C:147, pimpleFoamYade.C:109).  The reference calls
 * runTime.write() just BEFORE that (icoFoamYade.C:142, pimpleFoamYade.C:107), i.e. what it writes is the step's alpha / uSource.  With
 * hold = 1 the reset is deferred to the start of the next fy_solver_step (the same sequence), so that a caller can read or write
 * those fields in between. */
int fy_solver_hold_sources(fy_solver*, int hold);

/* fieldAverage on this solver (fy_average_desc above).  NULL or n_items 0: off, the buffers freed.  A new call starts every item from zero.  An unknown field,
 * a field this case does not have, a duplicate or more than FY_AVERAGE_MAX_ITEMS items: FY_ERR_INVALID naming the field; a slab solver: FY_ERR_UNSUPPORTED.
 * While it is on, "<field>Mean" [n][1|3] and "<field>Prime2Mean" [n][1|6] are names for fy_solver_field_count / _read_field_host / _write_field_host
 * (writing is how a restart loads them, together with fy_solver_set_average_state; it touches nothing else).  One launch per step on the solver's stream,
 * no host synchronisation; its time is the "field_average" clock of fy_solver_get_kernel_timing. */
int fy_solver_set_field_average(fy_solver*, const fy_average_desc*);
int fy_solver_get_average_state(fy_solver*, int item, int64_t* samples, double* time_averaged);
int fy_solver_set_average_state(fy_solver*, int item, int64_t samples, double time_averaged);

/* Run-time monitors on this solver (fy_monitor_desc above).  NULL or n_objects 0: off, the buffers freed; a new call starts every history from empty.  FY_ERR_INVALID,
 * naming the object and the word: an unknown field or operation, a field this case does not have, a weighted operation without its weight field, an empty side mask
 * (a patch without faces on a general mesh), more than FY_MONITOR_MAX_OBJECTS objects or FY_MONITOR_MAX_FIELDS fields; a slab solver: FY_ERR_UNSUPPORTED.
 * At most three launches per sampled step on the solver's stream and no host synchronisation; their time is the "monitors" clock of fy_solver_get_kernel_timing.
 * _layout: the number of values in a row of `object` and their labels, separated by '\n': "volAverage(p)", "volAverage(U)_x" ...
 * _get_monitor_rows: rows [first_row, first_row + max_rows) of the object's history since set_monitors: times[r], values[r][n_values]; *n_rows = how many were copied
 * (times and values may be NULL to count: *n_rows = rows from first_row on).  Only this call waits for the device.
 * Boundary values as the equations see them are field names of fy_solver_read_field_host / _field_count (read-only; a slab solver: FY_ERR_UNSUPPORTED):
 * "p_boundary" [nb], "U_boundary" [nb][3], "T_boundary" [nb] (thermal on); nb = 2 (ny nz + nx nz + nx ny), the six sides in the order x- x+ y- y+ z- z+, each side's
 * faces with the lower remaining axis fastest.  fixedValue: the value; zeroGradient: the owner cell's; slip / symmetry: the owner's, a vector without its normal
 * component; fixedFluxPressure: p_P + snGrad / deltaCoeff with the gradient as constrainPressure last left it. */
int fy_solver_set_monitors(fy_solver*, const fy_monitor_desc*);
int fy_solver_monitor_layout(fy_solver*, int object, int32_t* n_values, char* labels, int cap);
int fy_solver_get_monitor_rows(fy_solver*, int object, int64_t first_row, int64_t max_rows, double* times, double* values, int64_t* n_rows);

/* Wall loads on this solver (fy_wall_loads_desc above).  NULL or an all-zero descriptor: off, the buffers freed, nothing launched; a new call starts every history from
 * empty.  Objects are numbered forces[0 .. n_forces), then "wallShearStress", then "yPlus" (those that are on).  FY_ERR_INVALID, naming the object and the word: an empty
 * patch set (sides / patches), a side mask past 6 bits, more than FY_WALL_LOADS_MAX_FORCES objects or FY_WALL_LOADS_MAX_PATCHES patches, rho <= 0, a negative interval,
 * yPlus in a case with neither a turbulence model nor nu > 0; a slab solver: FY_ERR_UNSUPPORTED.  Two launches per sampled step (the face kernel, the fold) on the
 * solver's stream, no host synchronisation; their time is the "wall_loads" clock of fy_solver_get_kernel_timing (unknown while wall loads are off).
 * _layout / _get_wall_load_rows: as fy_solver_monitor_layout / fy_solver_get_monitor_rows; only _get_wall_load_rows waits for the device.  Patches are labelled x- x+ y-
 * y+ z- z+: "min(x-)_x" ... "max(x-)_z" (wallShearStress), "min(x-)" "max(x-)" "average(x-)" (yPlus).
 * Read-only field names while the object is on: "wallShearStress_boundary" [nb][3], "yPlus_boundary" [nb] in the order of "p_boundary", as the last sample left them
 * (zeros on faces outside the set).  Always: "nut_boundary" [nb] (nut on the boundary as the equations see it; zeros when laminar), "nearWallDist" [nb]. */
/* Inlets on this solver (fy_inlets_desc above).  NULL or n == 0: none, the buffers freed.  Allowed until the first step (afterwards FY_ERR_INVALID): the solver is left
 * as a create with these inlets would have left it -- the faces carry the value at start_time and the initial boundary flux is re-formed from the current U.
 * FY_ERR_INVALID by name: a term count outside 1 .. 3, an unknown function or shape kind, a table without points or with times that do not increase, frequency <= 0,
 * a per-face shape on a side without faces or without its array, a side that does not exist, is listed twice or is not FY_BC_U_FIXED_VALUE (fy_ldu_solver: a cyclic
 * patch has no faces).  FY_ERR_UNSUPPORTED: a slab solver; no patch fixes the pressure, no velocity patch is adjustable and a term's shape carries a net normal flux
 * (the rule of fy_solver_create's balance check).  "inlets" is a clock of fy_solver_get_kernel_timing while inlets are set. */
int fy_solver_set_inlets(fy_solver*, const fy_inlets_desc*);
int fy_solver_set_wall_loads(fy_solver*, const fy_wall_loads_desc*);
int fy_solver_wall_loads_layout(fy_solver*, int object, int32_t* n_values, char* labels, int cap);
int fy_solver_get_wall_load_rows(fy_solver*, int object, int64_t first_row, int64_t max_rows, double* times, double* values, int64_t* n_rows);

/* Porous zones (not in the reference, whose solvers carry no fvOptions; DESIGN.md section 3 "Porous zones", DESIGN_FV.md "Porous resistance").  A zone is a set of
 * cells in which the momentum equation gains an implicit resistance, diagonal in the global axes: per component q
 *     C_q(c) = nu d_q + 0.5 |U*_c| f_q        the left-hand side gains  a_c V_c C_q(c) U_c,q
 * d [1/m^2] and f [1/m] >= 0 (OpenFOAM's DarcyForchheimer coefficient mu D + rho |U| / 2 F per unit density, with a diagonal tensor, taken fully implicitly per
 * component: this library's own operator), a_c = alpha_c with pimpleFoamYade and 1 with icoFoamYade, nu the laminar viscosity, U* the velocity the matrix is assembled
 * around, |U| = sqrt((u0^2 + u1^2) + u2^2).  The coefficient joins the per-component diagonal a slip patch uses: the solve takes it per component, A() its component
 * mean, H() what a component has over the mean; UcEqn.relax() takes its component maximum into the dominance test.  The turbulence and T equations get no porous
 * source, the particle forces are untouched, and the `forces` object keeps leaving the porous contribution out.
 * set: NULL or n_zones == 0 removes the zones and frees what they held (every kernel then takes the path it took before); a set may be replaced between steps.
 * `cells` are solver cell labels (fy_solver: i + nx (j + ny k)).  FY_ERR_INVALID by name: more than FY_POROUS_MAX_ZONES zones, an empty zone, a label out of range,
 * a cell in two zones (or twice in one), a negative or non-finite coefficient, a null cell list.  FY_ERR_UNSUPPORTED: a slab solver (fy_solver_create_slab).
 * get_porous_stats: per zone z, from the CURRENT U and alpha, cells[z], volume[z] = S V, void_volume[z] = S a V and force[3 z + q] = S a V C_q(U) U_q (per unit
 * density: multiply by rho for newtons), each array [n_zones] ([n_zones][3]) or NULL; one kernel over the zones' cells on request, folded in a fixed order (the same
 * bits from run to run); the only porous call that waits for the device; its launches are the "porous_force" clock of fy_solver_get_kernel_timing (the step never
 * launches it: without a zone the clock counts nothing).  While zones are set, "porousZone" [n] (0: none, 1 + the zone's index; as doubles) and "mom_bd" [n][3] (the
 * momentum matrix's per-component diagonal: slip patches + zones, as the last assembly left it) are read-only field names; without zones both names and the
 * statistics are FY_ERR_INVALID. */
#define FY_POROUS_MAX_ZONES 8
typedef struct fy_porous_zone {
    char name[32];
    double d[3];                  /* Darcy coefficients [1/m^2], per global axis */
    double f[3];                  /* Forchheimer coefficients [1/m] */
    int32_t n_cells;
    const int32_t* cells;         /* [n_cells] solver cell labels; copied by the setter */
} fy_porous_zone;
typedef struct fy_porous_desc {
    int32_t n_zones;
    fy_porous_zone zones[FY_POROUS_MAX_ZONES];
} fy_porous_desc;
int fy_solver_set_porous_zones(fy_solver*, const fy_porous_desc*);
int fy_solver_get_porous_stats(fy_solver*, int32_t* n_zones, int64_t* cells, double* volume, double* void_volume, double* force);

/* Solid-phase statistics on this solver (not in the reference; DESIGN.md section 3 "Solid-phase statistics").  on != 0: once per step, after the T equation and before
 * fieldAverage and the monitors sample, one more scatter over the stencils of every located particle of EVERY batch forms eight sums per cell c (w: the stencil
 * weight, sum_c w = 1; point-force mode: the containing cell with w = 1; d = 2 r, Vp = pi d^3 / 6, Tp: the temperature the heat exchange holds for the particle at
 * the end of the step, s7 = 0 without heat transfer):
 *   s0 = sum w   s1 = sum w Vp   s2..s4 = sum (w Vp) v   s5 = sum (w Vp) |v|^2   s6 = sum w d^2   s7 = sum (w Vp) Tp
 * and from them, with the cell volume V (zeros where s1 == 0):
 *   nParticle = s0 / V [1/m^3]   solidFraction = s1 / V (unclamped; alpha stays what it is)   uSolid = s(2..4) / s1 [m/s]
 *   granularTemperature = max(0, (s5 / s1 - |uSolid|^2) / 3) [m^2/s^2]   dSauter = (6 / pi) s1 / s6 [m]   TParticle = s7 / s1 [K] (heat transfer on only)
 * While it is on, "solidMoments" [n][8] (s0 .. s7) and the six fields -- "uSolid" [n][3], the others [n] -- are names of fy_solver_field_count / _read_field_host
 * (read-only: writing is FY_ERR_INVALID), names fieldAverage and the volume monitors accept, and the pass's launches are the "solid_stats" clock of
 * fy_solver_get_kernel_timing.  They are zero before the first coupling call and describe the particles of the last one afterwards.  on == 0 (the default): nothing
 * is launched or allocated, the names are unknown; switching off frees the memory (16 doubles per cell, 17 with heat transfer).  FY_ERR_UNSUPPORTED: a slab solver
 * (fy_solver_create_slab); and fy_solver_step while fibre coupling is on. */
int fy_solver_set_solid_statistics(fy_solver*, int on);

/* Heat exchange (fy_case_desc.thermal.on; FY_ERR_INVALID on a solver without it).  The caller owns the particle temperatures: Tp[n] in the batch's wire order for the
 * n particles the batch holds now, host or device memory (copied), or NULL = thermal.particle_temperature for all of them; they stand until the next call for that
 * batch or until the batch's particle count changes (then the uniform value again).  q[n]: W into each particle over the last step, wire order, 0 for a particle
 * nobody located.  Stats of the last step: Jacobi passes and initial residual of the T solve, heat_to_particles_W = sum of q over all batches (summed on the device when asked for: pass NULL to skip it).
 * While thermal is on, "T" [n], "heatSp" [n] (W/K) and "heatSu" [n] (W) are field names of fy_solver_read/write_field_host (the sources: the last step's), "T" one that
 * fieldAverage accepts, and "heat_coeff", "heat_flux", "T_assemble" kernel clocks of fy_solver_get_kernel_timing; with thermal.beta != 0 and g != 0 also the field "buoyancy" [n][3]
 * (the acceleration the last step added to the momentum source) and the clock "buoyancy". */
int fy_solver_set_particle_temperatures_host(fy_solver*, int batch, const double* Tp);
int fy_solver_set_particle_temperatures_device(fy_solver*, int batch, const double* d_Tp);
int fy_solver_get_particle_heat_host(fy_solver*, int batch, double* q);
int fy_solver_get_thermal_stats(fy_solver*, int32_t* iterations, double* initial_residual, double* heat_to_particles_W);
/* The batch's particle temperatures as they stand now, Tp[n] in wire order for the n particles the batch holds (NULL: `batch` is not looked at), and the solver's count of resets (NULL: skip).
 * With thermal.particle_cp > 0 the library owns one Tp array per batch: made at the batch's first step from thermal.particle_temperature or from what
 * fy_solver_set_particle_temperatures_* gave (which then sets the CURRENT temperatures; NULL there re-initialises to the uniform value), advanced by every step, kept while
 * the batch's particle count is unchanged -- a particle's identity is its place in the wire order.  When the count changes the batch falls back to the uniform value and
 * the reset counter goes up by one.  With particle_cp == 0: what the caller set, or the uniform value.  FY_ERR_INVALID on a solver without heat transfer. */
int fy_solver_get_particle_thermal_state(fy_solver*, int batch, double* Tp, int64_t* resets);

/* ---- OpenFOAM case directories (what the reference's executables get from runTime / mesh / the field constructors, createFields.H
 * of both solvers, and give back with runTime.write()).  Supported subset: ONE axis-aligned blockMesh hex block of uniform cubes whose
 * six sides are covered by `boundary` patches; velocity patches fixedValue (uniform, or a nonuniform list: an inlet) / uniformFixedValue / flowRateInletVelocity (inlets, above) / noSlip / zeroGradient; pressure patches
 * zeroGradient / fixedValue (uniform) / fixedFluxPressure; internalField uniform or nonuniform; fixed deltaT.  Everything else is
 * refused with FY_ERR_UNSUPPORTED and a message naming file and keyword.
 *   system/blockMeshDict, system/controlDict, system/fvSolution (PISO | PIMPLE, solvers.p / pFinal / U),
 *   system/fvSchemes (must ask for Euler / Gauss linear / linear / corrected|orthogonal, div(phi,U) Gauss linear | upwind | linearUpwind grad(U):
 *   what the solver implements),
 *   constant/transportProperties (nu, partDensity, fluidDensity | continuousPhaseName + rho.<phase>), constant/g,
 *   <startTime>/U | U.<phase>, <startTime>/p */
typedef struct fy_foam_case fy_foam_case;
typedef struct fy_foam_case_info {
    double start_time, end_time, delta_t;
    int32_t write_interval_steps;          /* writeInterval in steps (writeControl timeStep, or runTime / deltaT) */
    int64_t n_cells;
    char u_name[64];                       /* "U" (icoFoamYade) or "U.<continuousPhaseName>" (pimpleFoamYade/createFields.H:35-45) */
    char phase[32];
    char start_name[32];                   /* name of the start time directory as written in controlDict */
    char patch_of_side[6][64];             /* blockMesh patch on the XMIN, XMAX, YMIN, YMAX, ZMIN, ZMAX side */
    int64_t field_cells, field_offset;     /* cells the field files (and fy_foam_case_initial_*, fy_foam_case_write_fields) hold, global number of the first:
                                              n_cells and 0, or one processor directory's slab (fy_foam_case_open_processor) */
    int32_t n_ignored_functions;           /* controlDict functions: objects of a type other than fieldAverage, volFieldValue, surfaceFieldValue -- accepted, never run (fy_foam_case_ignored_function) */
} fy_foam_case_info;
int fy_foam_case_open(const char* case_dir, int solver /* FY_SOLVER_ICO | FY_SOLVER_PIMPLE */, fy_foam_case** out);
/* a DECOMPOSED case (decomposePar, simple (1 1 nranks); the reference's -parallel run, README.md:29): mesh, controls and schemes from the case, the
   field files of <case>/processor<rank> -- its z-slab's cells in the global order, the processor patches kept as read and written back --; time
   directories go to the processor directory (reconstructPar's input).  fy_case_desc still describes the WHOLE block (fy_solver_create_slab) */
int fy_foam_case_open_processor(const char* case_dir, int solver, int rank, int nranks, fy_foam_case** out);
int fy_foam_case_desc(const fy_foam_case*, fy_case_desc* out);                   /* ready for fy_solver_create */
int fy_foam_case_info_get(const fy_foam_case*, fy_foam_case_info* out);
int fy_foam_case_initial_fields(const fy_foam_case*, double* U /* [n][3] or NULL */, double* p /* [n] or NULL */);
/* start-time nut.<phase> of a case with a turbulence model (hand it to fy_solver_write_field_host(s, "nut", ...) when it is not uniform) */
int fy_foam_case_initial_nut(const fy_foam_case*, double* nut /* [n] */);
int fy_foam_case_initial_k(const fy_foam_case*, double* k /* [n] */);          /* start-time k.<phase> of a kEqn / kEpsilon case */
int fy_foam_case_initial_epsilon(const fy_foam_case*, double* eps /* [n] */);  /* start-time epsilon.<phase> of a kEpsilon case */
/* heat transfer: constant/couplingProperties `heatTransfer { active on; nusseltModel RanzMarshall | Gunn; Cp; kappa; Prt; particleTemperature; }` (Gunn: pimpleFoamYade)
   becomes fy_case_desc.thermal, completed by <startTime>/T | T.<phase> (internalField uniform | nonuniform; patches zeroGradient | fixedValue uniform), divSchemes
   div(phi,T) | div(alphaPhic,T) = [bounded] Gauss linear | upwind and fvSolution solvers.T | T.<phase>.  Refused by name (FY_ERR_UNSUPPORTED): an unknown model or
   entry, Gunn with icoFoamYade, a missing Cp / kappa / temperature file / solvers entry, another patch type, a general-mesh or decomposed case.  fy_foam_case_write_time
   writes the solver's T beside the other fields; fy_foam_case_initial_T hands out the start time's (for fy_solver_write_field_host(s, "T", ...)) */
int fy_foam_case_initial_T(const fy_foam_case*, double* T /* [n] */);
/* runTime.write(): <case>/<time_name>/{U | U.<phase>, p [, alpha.<phase>]} as ASCII volFields with the case's own patch entries */
int fy_foam_case_write_time(const fy_foam_case*, fy_solver*, const char* time_name);
/* the same from host arrays over the WHOLE block (a slab run gathers its ranks' owned cells first: foamYadeHip_mpi -parallel); alpha / nut / k / epsilon
   may be NULL where the case has no such field */
int fy_foam_case_write_fields(const fy_foam_case*, const char* time_name, const double* U, const double* p, const double* alpha, const double* nut,
                              const double* k, const double* epsilon);
/* controlDict `functions` [OF-6 functionObjectList]: ONE entry of `type fieldAverage` (not `enabled false`) becomes fy_case_desc.average / fy_ldu_case.average:
 * fields ( <file name> { mean on|off; prime2Mean on|off; base time|iteration; } ... ) with the case's file names (U | U.<phase>, p, alpha.<phase>, nut.<phase>,
 * k.<phase>, epsilon.<phase>, uParticle, uSource), timeStart / timeEnd (start_after = max(0, timeStart - startTime)), writeControl absent | writeTime | outputTime,
 * executeControl absent | timeStep (interval 1), restartOnRestart.  Refused by name (FY_ERR_UNSUPPORTED): window, restartOnOutput on, periodicRestart on, an
 * unknown field, a field the case does not have, mean off with prime2Mean on, another base, a second fieldAverage.  Objects of every other type are accepted
 * and NOT run: the i-th one's "<name> (type <type>)" for a caller that wants to say so.
 * fy_foam_case_write_time / _write_time_ldu of a solver with averaging on also write <file name>Mean (the base field's class, dimensions and patch entries),
 * <file name>Prime2Mean (volScalarField | volSymmTensorField, squared dimensions, calculated patches) and <time>/uniform/<object>Properties (per field
 * totalIter = N + 1, totalTime = T + deltaT: OpenFOAM's convention as recalled, unpinned).  fy_foam_case_restore_averages (_ldu for a general case) loads them back from the start time
 * directory into a new solver (restartOnRestart off, and the files there); *restored = the number of items loaded, 0 = averaging starts from zero. */
int fy_foam_case_ignored_function(const fy_foam_case*, int i, char* out, int cap);
/* controlDict `functions`, objects of `type volFieldValue` / `type surfaceFieldValue` (not `enabled false`) become fy_case_desc.monitors / fy_ldu_case.monitors, in the
 * dictionary's order ([OF-6 fieldValue, volFieldValue, surfaceFieldValue] as recalled, unpinned).  Accepted: fields ( <file name> ... ) with the case's file names (volume: what
 * fieldAverage takes; surface: phi, p, U | U.<phase>, T), operation (fy_monitor_desc's words), weightField alpha.<phase> (volume) | phi (surface), regionType all (volume) |
 * regionType patch with name <patch> (surface; on a block the patch becomes its mask of sides), writeFields false, writeControl / executeControl timeStep with writeInterval /
 * executeInterval N (one sample every N steps), enabled, libs, log.  Refused by name with the accepted words (FY_ERR_UNSUPPORTED): every other keyword (scaleFactor,
 * postOperation, ...), regionType cellZone | faceZone | sampledSurface, writeFields true, other controls, unknown operations, fields and patches, a cyclic patch, a decomposed case.
 * fy_foam_case_write_monitors (_ldu for a general case) appends the rows the solver has gathered since the last call to
 * <case>/postProcessing/<object>/<start time name>/volFieldValue.dat | surfaceFieldValue.dat: '#' header lines (region type and name, number of cells | faces, total volume |
 * area, the column labels), then one row per sample: the time and the values, a vector as (x y z), writePrecision digits.  The first call of a run creates the file: a
 * restarted run writes into the directory of its own start time */
int fy_foam_case_monitor_count(const fy_foam_case*);
int fy_foam_case_write_monitors(const fy_foam_case*, fy_solver*);
/* controlDict `functions`, objects of `type forces | wallShearStress | yPlus` (not `enabled false`) become fy_case_desc.wall_loads / fy_ldu_case.wall_loads ([OF-6 forces,
 * wallShearStress, yPlus] as recalled, unpinned).  forces: patches ( <name> ... ), rho rhoInf with rhoInf <value>, pRef (default 0), CofR (x y z); accepted and unused: p, U,
 * log, libs, enabled, writeControl | executeControl timeStep with writeInterval | executeInterval N (one sample every N steps).  wallShearStress, yPlus: an optional patches
 * list, default every patch of type wall; one object of each.  Refused by name with the accepted words (FY_ERR_UNSUPPORTED): every other keyword (porosity, binData,
 * coordinateSystem, directForceDensity, ...), a rho other than rhoInf, other controls, an unknown or cyclic patch, more than FY_WALL_LOADS_MAX_FORCES forces objects or
 * FY_WALL_LOADS_MAX_PATCHES patches, a decomposed case.  The solver numbers the objects forces first (in the dictionary's order), then wallShearStress, then yPlus.
 * fy_foam_case_write_wall_loads (_ldu for a general case) appends the rows the solver has gathered since the last call to <case>/postProcessing/<object>/<start time
 * name>/forces.dat (time, then Fp Fv Mp Mv as (x y z)) | wallShearStress.dat (per patch a line: time, patch, min vector, max vector) | yPlus.dat (per patch: time, patch,
 * min, max, average): '#' header lines first, writePrecision digits; a block's patch that covers several sides has one line per side, named <patch>:<side> (x- .. z+).  The
 * first call of a run creates the file: a restarted run writes into the directory of its own start time */
int fy_foam_case_wall_loads_count(const fy_foam_case*);
int fy_foam_case_write_wall_loads(const fy_foam_case*, fy_solver*);
int fy_foam_case_restore_averages(const fy_foam_case*, fy_solver*, int* restored);
int fy_foam_case_close(fy_foam_case*);

/* ---- kernel-level entry points used by the roofline bench and the operator parity tests ------------------ */
/* y = A x for the symmetric 7-point pressure matrix (diag, ux, uy, uz) currently held by the solver; x,y host arrays */
int fy_solver_apply_p_matrix_host(fy_solver*, const double* x, double* y);
/* solve  A x = rhs  with the pressure solver of the case (PCG + multigrid / Jacobi, pFinal tolerances) and the pressure matrix the last
   step assembled; x holds the start vector on entry.  For known-answer tests of the solver itself (manufactured Poisson problems). */
int fy_solver_solve_p_host(fy_solver*, const double* rhs, double* x, int* iterations);
/* z = M^-1 r on the owned cells with the preconditioner of the case's p_solver and the pressure matrix the last step assembled: one multigrid V-cycle
   (FY_PSOLVER_PCG_MG), or r / diag (FY_PSOLVER_PCG_JACOBI); r, z host arrays.  On z-slabs the call is collective and takes the route the solve takes (the
   communication-avoiding cycle where the slabs carry its ghost planes).  The solver is left as it was found -- p, the residual, the carried sum of p, the
   levels' buffer roles: a run with calls between its steps gives the bits of a run without.  For tests that hold the cycle to a reference as an operation. */
int fy_solver_precondition_host(fy_solver*, const double* r, double* z);
/* the multigrid hierarchy of FY_PSOLVER_PCG_MG, finest first (one level with the Jacobi preconditioner): edge lengths, nz_owned = this rank's planes of a
   distributed level or every plane of a replicated one, distributed = 1 | 0; fills the first `cap` levels, *n_levels = how many there are.  The operators of
   level l >= 1 are read by name through fy_solver_read_field_host: mg<l>_diag | mg<l>_ux | mg<l>_uy | mg<l>_uz (nx ny nz_owned values; read-only), beside
   level 0's p_diag | p_ux | p_uy | p_uz. */
int fy_solver_mg_levels(fy_solver*, int cap, int32_t* nx, int32_t* ny, int32_t* nz_owned, int32_t* distributed, int* n_levels);
/* time `reps` launches of the pEqn Laplacian apply (the roofline kernel) with HIP events on the solver stream; returns avg ms */
int fy_solver_time_p_apply(fy_solver*, int reps, double* avg_ms);

/* ======================================================================================================== */
/* Multi-GPU: z-slab decomposition of the block, one slab per rank.                          */
/* ======================================================================================================== */
/* A communicator carries the neighbour exchanges (FV halos 1 plane, particle halos 5 planes, reverse sums), the tiny all-reduces
 * (Krylov scalars, Courant number, continuity errors) and the all-gather of the coarse multigrid level.
 *   fy_comm_create_rccl        one process per GPU over RCCL/xGMI; `id128` = the 128 bytes from fy_rccl_unique_id() on rank 0,
 *                              distributed by the launcher (bench.py uses torch.distributed for that)
 *   fy_comm_create_local_group n "virtual slabs" inside ONE process (one host thread per slab, device-to-device copies): the same
 *                              solver code, used to test the decomposition on a single-GPU box
 * The reference's equivalent is OpenFOAM's own domain decomposition (`-parallel`, README.md:29) [OF-6, not in the reference]. */
typedef struct fy_comm fy_comm;
int fy_rccl_unique_id(void* out128);
int fy_comm_create_rccl(int rank, int size, const void* id128, int device_ordinal, fy_comm** out);
int fy_comm_create_local_group(int n, fy_comm** out /* [n] */);
/* host-staged communicator: the library moves the planes device -> pinned host -> callback -> device and leaves the transport between the
   processes to the caller (MPI, gloo, pipes ...).  One process per slab like RCCL, so the ORDER in which separate processes reach the
   collectives is real -- what the in-process group cannot show -- on machines where RCCL cannot run (one GPU shared by the ranks).
   Callbacks return 0 on success; all buffers are host memory; a missing neighbour's buffers are NULL with count 0. */
typedef struct fy_comm_callbacks {
    void* user;
    /* send n_up doubles to rank+1 and n_down to rank-1; receive m_down from rank-1 and m_up from rank+1 (any of them may be 0) */
    int (*sendrecv)(void* user, const double* send_up, size_t n_up, double* recv_from_down, size_t m_down, const double* send_down, size_t n_down,
                    double* recv_from_up, size_t m_up);
    int (*allreduce)(void* user, double* buf, int n, int is_max);                       /* in place, identical result on every rank */
    int (*allgather)(void* user, const double* send, double* recv, size_t count_per_rank);
} fy_comm_callbacks;
int fy_comm_create_host(int rank, int size, const fy_comm_callbacks* cb, fy_comm** out);
/* One process per slab with DIRECT PEER STORES (SURVEY.md 8e "prefer direct peer stores over the fully connected xGMI mesh"; stands where the reference's
 * per-particle collectives stand, FoamYade.C:228, 511-515, and where OpenFOAM's processor patches exchange halos): every rank exports one device window
 * (hipIpcGetMemHandle) and maps the others'; a neighbour exchange is a copy kernel whose stores land in the neighbour's window + a flag, an all-reduce of
 * <= 32 doubles ONE kernel that stores this rank's values into every peer's window and folds in rank order.  The callbacks carry the bootstrap only
 * (allgather of the 64-byte handles, allreduce as the closing barrier); sendrecv may be NULL.  Works for the GPUs of one xGMI node and for N processes that
 * share ONE GPU (where RCCL refuses to run): select with FOAMYADE_COMM=ipc in bench.py.  At most 8 ranks.
 * FOAMYADE_IPC_SLOT_MB (default 8): bytes per neighbour slot (larger groups travel in chunks); FOAMYADE_IPC_TIMEOUT_MS (default 20000): bound of every
 * device-side wait -- a peer that never arrives becomes FY_ERR_TRANSPORT at the next call instead of a hung GPU. */
int fy_comm_create_ipc(int rank, int size, const fy_comm_callbacks* cb, int device_ordinal, fy_comm** out);
/* diagnostic: calls made through this communicator so far: {neighbour exchanges, all-reduces, all-gathers, bytes sent to neighbours} */
int fy_comm_stats(fy_comm*, uint64_t* out4);
/* the same call counts by the solver phase that issued them, as text: one line "<phase> <exchanges> <all-reduces> <all-gathers>" per phase
 * (step_start, particle, momentum, momentum_solve, corrector, p_operators, pcg, vcycle, turbulence ...); the per-step collective budget
 * of the slab solver is asserted on these (tests/test_slabs.py) */
int fy_comm_stats_by_tag(fy_comm*, char* buf, size_t cap);
/* collective known-answer run of every operation the slab solver uses on this communicator (a grouped two-field neighbour exchange, sum and
 * max all-reduce, all-gather); bench.py runs it in throw-away processes before it commits a multi-GPU run to the communicator */
int fy_comm_selftest(fy_comm*, int device_ordinal);
int fy_comm_destroy(fy_comm*);
int fy_comm_rank(fy_comm*);
int fy_comm_size(fy_comm*);
/* `c` describes the GLOBAL block; rank r owns z-planes [r*nz/size, (r+1)*nz/size) (nz/size must be even and >= the particle halo).
 * Collective: every rank of the communicator must call it, and later fy_solver_step, together.  Field accessors then address the
 * rank's OWNED cells only.  Each rank is given the particles that lie inside its own slab. */
int fy_solver_create_slab(const fy_case_desc* c, const fy_transport* transport, int device_ordinal, fy_comm* comm, fy_solver** out);
int fy_solver_local_cells(fy_solver*);

/* per-kernel HIP-event clocks on the solver stream, accumulated over steps since the last enable(1):
 * kernel = "mg_smooth_l0" (pEqn Laplacian apply fused with the damped-Jacobi update, fine level), "p_apply_dot" (pEqn Laplacian
 * apply + p.Ap inside PCG), "mom_pass" (fused momentum Jacobi pass), "mom_assemble" (the momentum assembly sweep, one sample per outer iteration; only with enable(2), which switches on this clock beside the others: an
 * event pair idles the stream for some microseconds, and the step's other clocks were measured without it), "porous_force"
 * (k_porous_force and its fold: launched by fy_solver_get_porous_stats only, so without a zone it counts no launch) */
int fy_solver_enable_kernel_timing(fy_solver*, int on);
int fy_solver_get_kernel_timing(fy_solver*, const char* kernel, double* total_ms, int64_t* launches);
/* z-slabs: how long the solver's stream sat WAITING for slab exchanges, by phase {step start, particle, momentum, corrector}, accumulated since the
 * call that switched the clock on.  With the exchanges overlapped (the default; FOAMYADE_HALO_OVERLAP=0 switches to exchange-then-consume) a wait
 * runs from the end of the interior planes' sweep to the arrival of the ghost planes; in the serial schedule it is the exchange itself.  The clock
 * costs an event pair per exchange (5 - 10 us of idle stream each): off by default.  (The particle phase's exchanges run inside the coupling object
 * and are not sampled here.) */
int fy_solver_enable_exchange_timing(fy_solver*, int on);
int fy_solver_get_exchange_wait(fy_solver*, double ms[4], int64_t waits[4]);


/* ------------------------------------------------------------------------------------------------------------------------------------
 * icoFoamYade and pimpleFoamYade on a GENERAL polyhedral mesh (round 4).  The reference's solvers run on whatever createMesh.H
 * hands them (icoFoamYade/icoFoamYade.C:42, pimpleFoamYade/pimpleFoamYade.C:47) and carry non-orthogonal corrector loops (icoFoamYade.C:114-131,
 * pEqn.H:24-47); fy_solver above is the structured block.  fy_ldu_solver takes the mesh in OpenFOAM's own addressing -- constant/polyMesh: points,
 * faces, owner, neighbour, boundary -- builds OpenFOAM's geometry from it (face triangle / cell pyramid decomposition, linear weights,
 * nonOrthDeltaCoeffs, nonOrthCorrectionVectors, fvc::reconstruct's tensors [OF-6]) and runs the loop bodies with owner / neighbour (LDU) addressing:
 * Euler ddt, Gauss linear | upwind | linearUpwind | limited (NVD / TVD) div, Gauss linear grad, Gauss linear CORRECTED laplacian (the explicit non-orthogonal part is what the
 * correctNonOrthogonal loop iterates on), PCG in its single-reduction form with the diagonal or an agglomeration-multigrid preconditioner (p_solver),
 * Jacobi sweeps for U.  Patches: fixedValue / zeroGradient / symmetry (slip) for U (noSlip = fixedValue 0), translational cyclic pairs; zeroGradient / fixedValue for p, fixedFluxPressure with
 * pimpleFoamYade.  pimpleFoamYade (fy_ldu_case.solver): Gaussian 4-way coupling, the void-fraction-weighted UcEqn / pEqn, gravity, PIMPLE outer correctors,
 * relaxation, adjustable time step, laminar Stokes stress, LES Smagorinsky / kEqn or RAS kEpsilon, with nutkWallFunction / epsilonWallFunction patches (nearWallDist on any face).  The coupling object (fy_ldu_solver_coupling) works on the mesh's own
 * cell centres and volumes: explicit k-d tree, and for the point-force locate (mesh.findCell, FoamYade.C:251) the nearest centre followed by a walk
 * across the faces the point lies outside of. */
typedef struct fy_poly_mesh {
    int32_t n_points;
    const double* points;            /* [n_points][3] */
    int32_t n_faces, n_internal_faces;
    const int32_t* face_offsets;     /* [n_faces + 1] into face_points */
    const int32_t* face_points;      /* a face's points turn counter-clockwise seen from outside its owner */
    const int32_t* owner;            /* [n_faces] */
    const int32_t* neighbour;        /* [n_internal_faces]: internal faces first, owner < neighbour */
    int32_t n_cells;
    int32_t n_patches;
    const int32_t* patch_start;      /* [n_patches] first face of the patch (>= n_internal_faces) */
    const int32_t* patch_size;
    const int32_t* patch_neighbour;  /* NULL, or per patch: the index of its cyclic partner (constant/polyMesh/boundary: type cyclic; neighbourPatch), -1 for an ordinary
                                        patch.  Translational cyclics whose faces match one to one, in order [OF-6 cyclicPolyPatch]: each pair becomes one more internal
                                        face of the solver, numbered after the mesh's own (fy_ldu_solver_read_field_host "orig_face" maps the solver's faces to the
                                        caller's); the patches themselves are left without faces, their entries in the per-patch arrays unused */
} fy_poly_mesh;
/* Flow-rate control for periodic domains: the role of OpenFOAM's meanVelocityForce fvOption (the arithmetic is OpenFOAM-6's meanVelocityForce.C as recalled, unpinned:
 * DESIGN.md section 3 "Flow-rate control").  A uniform pressure gradient G along flowDir = ubar / |ubar| is adjusted so that the bulk velocity stays |ubar|.  Device state:
 * gradP0 (starts at gradient0) and dGradP (starts at 0).  Per momentum assembly: gradP0 += dGradP, dGradP = 0, and flowDir * gradP0 joins the external momentum source
 * (what "uSource" holds, which still reads back as written).  After every corrector's velocity update, with w_i = 1 (superficial: alpha_i) and V the mesh volume:
 *     ubar = (S (flowDir . U_i) w_i V_i) / V     rAUave = (S rAU_i w_i V_i) / V     dGradP = relaxation (|ubar| - ubar) / rAUave     U_i += flowDir (rAU_i dGradP)
 * dGradP is assigned, not accumulated (OpenFOAM's behaviour, kept); phi is left alone.  The sums are block partials folded in a fixed order: FP64, no atomics, the same
 * bits from run to run.  At most three launches per corrector and one per assembly on the solver's stream, no host synchronisation; their time is the "flow_control"
 * clock of fy_ldu_solver_get_kernel_timing. */
typedef struct fy_flow_control_desc {
    int32_t on;
    double ubar[3];                  /* the bulk velocity to hold; |ubar| > 0 */
    double relaxation;               /* in [0, 1]; OpenFOAM's default is 1 */
    double gradient0;                /* the pressure gradient to start from (a restart: <time>/uniform/meanVelocityForceProperties) */
    int32_t superficial;             /* pimpleFoamYade only: weigh both sums with the void fraction (0: OpenFOAM's definition) */
} fy_flow_control_desc;
typedef struct fy_ldu_case {
    double dt, nu, rho_fluid, rho_particle;
    int32_t n_correctors, n_non_orth_correctors, momentum_predictor, p_ref_cell;
    double p_ref_value;
    double p_tol, p_rel_tol, p_final_tol, p_final_rel_tol; int32_t p_max_iter;
    double u_tol, u_rel_tol; int32_t u_max_iter;
    int32_t p_solver;                /* FY_PSOLVER_PCG_JACOBI: PCG.C with the diagonal preconditioner | FY_PSOLVER_PCG_MG: preconditioned by an agglomeration
                                        multigrid V-cycle (fvSolution: solver / preconditioner GAMG) built from the face areas like faceAreaPair */
    const int32_t* u_bc;             /* per patch: FY_BC_U_FIXED_VALUE | FY_BC_U_ZERO_GRADIENT | FY_BC_U_SLIP (symmetryPlane / symmetry / slip: each face with its own normal) |
                                        FY_BC_U_INLET_OUTLET | FY_BC_U_PRESSURE_INLET_OUTLET (open boundaries, below) */
    const double* u_value;           /* [n_patches][3]; the inlet value of an FY_BC_U_INLET_OUTLET patch */
    const int32_t* p_bc;             /* per patch: FY_BC_P_ZERO_GRADIENT | FY_BC_P_FIXED_VALUE */
    const double* p_value;           /* [n_patches] */
    /* pimpleFoamYade on the general mesh (solver = FY_SOLVER_PIMPLE; pimpleFoamYade.C:60-114, UcEqn.H, pEqn.H): Gaussian 4-way coupling, the void-fraction-
     * weighted equations, laminar Stokes stress; p patches may then be FY_BC_P_FIXED_FLUX (fixedFluxPressure) too */
    int32_t solver;                  /* FY_SOLVER_ICO (the default) | FY_SOLVER_PIMPLE */
    int32_t n_outer_correctors;
    double g[3];
    double u_relax, u_relax_final, p_relax, p_relax_final;      /* relaxationFactors; <= 0: no entry (relax() does nothing) */
    int32_t adjust_time_step;        /* pimpleFoamYade only (pimpleFoamYade.C:62-64: readTimeControls.H, CourantNo.H, setDeltaT.H) */
    double max_co, max_delta_t;
    /* continuousPhaseTurbulence (pimpleFoamYade only): FY_TURBULENCE_LAMINAR | FY_TURBULENCE_SMAGORINSKY | FY_TURBULENCE_KEQN (LES, delta cubeRootVol) | FY_TURBULENCE_KEPSILON as in fy_case_desc */
    int32_t turbulence_model;
    double les_ck, les_ce, les_delta_coeff, nut_initial;
    const int32_t* nut_bc;           /* per patch: FY_BC_NUT_ZERO_GRADIENT | FY_BC_NUT_FIXED_VALUE (NULL: zeroGradient everywhere); FY_BC_WALL_FUNCTION (nutkWallFunction)
                                        with kEqn / kEpsilon: the file's value until the first correctNut(), nu (y+ kappa / ln(E y+) - 1) above yPlusLam afterwards,
                                        y+ = Cmu^1/4 y sqrt(k_P) / nu with y the face's nearWallDist (wf_kappa, wf_E below) */
    const double* nut_value;         /* [n_patches] */
    int32_t convection_scheme;       /* FY_CONVECTION_LINEAR (default) .. FY_CONVECTION_QUICK for div(phi,U) / div(alphaPhic,Uc), as fy_case_desc.convection_scheme */
    double convection_limiter_k;     /* limitedLinear's coefficient in [0, 1] */
    /* turbulence_model FY_TURBULENCE_KEQN (LES kEqn, DPMTurbulenceModels.C:76-77): the 0/k file (k_initial uniform; per patch FY_BC_NUT_ZERO_GRADIENT | _FIXED_VALUE),
     * div(alphaPhic,k) (FY_CONVECTION_LINEAR | _UPWIND), solvers.k, relaxationFactors equations k (<= 0: none); nut patches may then be FY_BC_NUT_CALCULATED
     * (the file's value until the first correctNut(), Ck sqrt(k_b) delta afterwards) */
    double k_initial;
    const int32_t* k_bc;             /* NULL: zeroGradient everywhere; FY_BC_NUT_INLET_OUTLET: k_value where the flux enters */
    const double* k_value;
    /* k_convection_scheme and eps_convection_scheme (below) -- fy_case_defaults: FY_CONVECTION_UPWIND; fy_ldu_case_defaults: FY_CONVECTION_LINEAR.
     * THE TWO DEFAULTS DIFFER: a case that runs on both solvers, or is compared across them, names both schemes */
    int32_t k_convection_scheme;
    double k_tol, k_rel_tol; int32_t k_max_iter;
    double k_relax;
    /* turbulence_model FY_TURBULENCE_KEPSILON (RAS kEpsilon, DPMTurbulenceModels.C:70-71): the coefficients, the 0/epsilon file and its controls as in fy_case_desc;
     * k as above (kqRWallFunction = FY_BC_NUT_ZERO_GRADIENT); a FY_BC_NUT_CALCULATED nut patch then carries Cmu k_b^2 / epsilon_b.  eps_bc FY_BC_WALL_FUNCTION
     * (epsilonWallFunction, the patch's nut a nutkWallFunction): each cell with such faces has its epsilon imposed, (1/W) sum Cmu^3/4 k^3/2 / (kappa y), and its
     * production replaced by (1/W) sum (nut_w + nu) |snGrad U| Cmu^1/4 sqrt(k) / (kappa y) over its W faces on those patches, y the faces' nearWallDist */
    double ras_cmu, ras_c1, ras_c2, ras_c3, ras_sigmak, ras_sigmaeps;      /* fy_ldu_case_defaults: 0.09, 1.44, 1.92, 0, 1, 1.3 */
    double eps_initial;
    const int32_t* eps_bc;           /* NULL: zeroGradient everywhere; FY_BC_NUT_INLET_OUTLET: eps_value where the flux enters */
    const double* eps_value;
    int32_t eps_convection_scheme;   /* default: see k_convection_scheme */
    double eps_tol, eps_rel_tol; int32_t eps_max_iter;
    double eps_relax;
    double wf_kappa, wf_E;          /* the wall functions' constants [OF-6 nutkWallFunction]; fy_ldu_case_defaults: 0.41, 9.8 */
    int32_t drag_law;                /* constant/couplingProperties as in fy_case_desc: FY_DRAG_* and FY_FORCE_* flags, zero = the reference's behaviour */
    uint32_t force_models;
    fy_average_desc average;         /* controlDict functions: the fieldAverage object as in fy_case_desc (all zero: none), applied at fy_ldu_solver_create */
    /* The fluid temperature equation and the particle-fluid heat exchange as in fy_case_desc.thermal (all zero: off -- nothing allocated, nothing launched).  Everything
     * of fy_thermal_desc applies but its six-sided T_bc[6] / T_value[6], which are NOT READ on a general mesh: the patch conditions are the two arrays below.  The
     * diffusion term is Gauss linear corrected like every laplacian here: gam_f = alphaf_f (D + nut / prt)_f |Sf|, implicit part gam_f dcNO_f, explicit part
     * gam_f (kvec_f . (grad T_old)_f) added to the owner and taken from the neighbour; the Gaussian scatter of Sp / Su goes out as FP64 global atomics (no tiles) */
    fy_thermal_desc thermal;
    const int32_t* T_bc;             /* per patch: FY_BC_T_ZERO_GRADIENT | FY_BC_T_FIXED_VALUE | FY_BC_T_INLET_OUTLET (NULL: zeroGradient everywhere); a symmetry / slip patch takes
                                        FY_BC_T_ZERO_GRADIENT, folded cyclic pairs are internal faces and need nothing */
    const double* T_value;           /* [n_patches] */
    fy_monitor_desc monitors;        /* controlDict functions: the volFieldValue / surfaceFieldValue objects as in fy_case_desc (all zero: none); `patch` is a patch index */
    int32_t solid_stats;             /* the solid-phase statistics as in fy_case_desc, applied with fy_ldu_solver_set_solid_statistics (0: off) */
    fy_flow_control_desc flow_control;      /* flow-rate control (all zero: off -- nothing allocated, nothing launched), applied at fy_ldu_solver_create */
    fy_inlets_desc inlets;                  /* inlets on fixed-value velocity patches as in fy_case_desc (all zero: none), applied with fy_ldu_solver_set_inlets */
    fy_wall_loads_desc wall_loads;          /* the forces / wallShearStress / yPlus objects as in fy_case_desc (all zero: none); a patch set is patches[0 .. n_patches) */
} fy_ldu_case;
typedef struct fy_ldu_solver fy_ldu_solver;
void fy_ldu_case_defaults(fy_ldu_case*);        /* the icoFoam cavity tutorial's controls (as fy_case_defaults); the patch arrays stay NULL */
int fy_ldu_solver_create(const fy_poly_mesh*, const fy_ldu_case*, const fy_transport* transport /* or NULL */, int device_ordinal, fy_ldu_solver** out);
int fy_ldu_solver_step(fy_ldu_solver*);                                     /* one pass of icoFoamYade.C:65-149 */
int fy_ldu_solver_get_stats(fy_ldu_solver*, fy_step_stats* out);
/* fieldAverage as on fy_solver (fy_solver_set_field_average): alpha, uParticle with pimpleFoamYade; uSource is what the coupling left (+ an external source
   with pimpleFoamYade, as the equations saw it); the same "<field>Mean" / "<field>Prime2Mean" field names */
int fy_ldu_solver_set_field_average(fy_ldu_solver*, const fy_average_desc*);
int fy_ldu_solver_get_average_state(fy_ldu_solver*, int item, int64_t* samples, double* time_averaged);
int fy_ldu_solver_set_average_state(fy_ldu_solver*, int item, int64_t samples, double time_averaged);
/* Run-time monitors as on fy_solver (fy_solver_set_monitors): a surface object's `patch` is a patch index (a folded cyclic patch has no faces and is refused by name).
 * "p_boundary" [nb], "U_boundary" [nb][3] and, with thermal on, "T_boundary" [nb] are read-only field names: nb = n_faces - n_internal_faces in the solver's
 * boundary-face order, like "nut_boundary" */
int fy_ldu_solver_set_monitors(fy_ldu_solver*, const fy_monitor_desc*);
int fy_ldu_solver_monitor_layout(fy_ldu_solver*, int object, int32_t* n_values, char* labels, int cap);
int fy_ldu_solver_get_monitor_rows(fy_ldu_solver*, int object, int64_t first_row, int64_t max_rows, double* times, double* values, int64_t* n_rows);
/* Wall loads as on fy_solver (fy_solver_set_wall_loads): a patch set is a list of patch indices, labelled "patch<index>"; a cyclic patch (folded into internal faces) or
 * a patch that does not exist is refused by name (FY_ERR_INVALID).  delta = deltaCoeffs of the boundary face ("dcNO"), y = nearWallDist, which is then formed for the
 * selected patches as well as for the wall-function patches.  "wallShearStress_boundary" [nb][3], "yPlus_boundary" [nb] in the solver's boundary-face order; the clock
 * is "wall_loads" of fy_ldu_solver_get_kernel_timing. */
/* Inlets as on fy_solver (fy_solver_set_inlets): `patch` is a patch index, a per-face shape follows the patch's faces in the solver's boundary-face order; the clock
 * is "inlets" of fy_ldu_solver_get_kernel_timing. */
int fy_ldu_solver_set_inlets(fy_ldu_solver*, const fy_inlets_desc*);
int fy_ldu_solver_set_wall_loads(fy_ldu_solver*, const fy_wall_loads_desc*);
int fy_ldu_solver_wall_loads_layout(fy_ldu_solver*, int object, int32_t* n_values, char* labels, int cap);
int fy_ldu_solver_get_wall_load_rows(fy_ldu_solver*, int object, int64_t first_row, int64_t max_rows, double* times, double* values, int64_t* n_rows);
/* Solid-phase statistics as on fy_solver (fy_solver_set_solid_statistics): the same sums, fields and names; a general mesh has no tiles, so the Gaussian scatter goes
 * out as FP64 global atomics.  The pass's launches are the "solid_stats" clock (beside "flow_control", below) of fy_ldu_solver_get_kernel_timing, switched on and reset by
 * fy_ldu_solver_enable_kernel_timing. */
int fy_ldu_solver_set_solid_statistics(fy_ldu_solver*, int on);
int fy_ldu_solver_enable_kernel_timing(fy_ldu_solver*, int on);
int fy_ldu_solver_get_kernel_timing(fy_ldu_solver*, const char* kernel, double* total_ms, int64_t* launches);
/* Flow-rate control (fy_flow_control_desc above).  set: NULL or on == 0 switches it off and frees its memory; every call with on != 0 restarts the state from gradient0.
 * FY_ERR_INVALID naming the entry for |ubar| = 0 or not finite, a relaxation outside [0, 1] or not finite, superficial with icoFoamYade.  get: the numbers of the last
 * correction -- gradient = gradP0 + dGradP, the uncorrected bulk velocity, the mean rAU, dGradP, the corrections so far; any pointer may be NULL; FY_ERR_INVALID while
 * the option is off.  Only this call waits for the device.  While the option is on, "flow_control" is a second clock of fy_ldu_solver_get_kernel_timing. */
int fy_ldu_solver_set_flow_control(fy_ldu_solver*, const fy_flow_control_desc*);
int fy_ldu_solver_get_flow_control(fy_ldu_solver*, double* gradient, double* ubar_uncorrected, double* rAU_ave, double* dGradP, int64_t* corrections);
/* Open boundaries (a side where fluid may leave or come back in, face by face): u_bc FY_BC_U_INLET_OUTLET | FY_BC_U_PRESSURE_INLET_OUTLET, k_bc / eps_bc
 * FY_BC_NUT_INLET_OUTLET, T_bc FY_BC_T_INLET_OUTLET; from a case directory the words inletOutlet (inletValue uniform ...) and pressureInletOutletVelocity.  The inlet
 * value travels in u_value / k_value / eps_value / T_value.  One byte per boundary face, the inflow mask (phi < 0), selects -- never blends -- per face: an inflow face
 * is the patch's fixedValue face (pressureInletOutletVelocity: U_b = n (n . U_P), the directionMixed form with value fraction I - n n in the matrix), an outflow face a
 * zeroGradient face.  An open velocity patch never fixes the flux: phiHbyA takes HbyA's cell value there and adjustPhi may scale it.  The mask is renewed on the device
 * (a) at the start of a step, (b) after each corrector's flux update, before the velocity is corrected or reconstructed, (c) after createPhi at create, at
 * fy_ldu_solver_set_inlets and at fy_ldu_solver_write_field_host("U"), which form phi with every open face evaluated as zeroGradient first.  "U_open_inflow" [nb] is
 * the mask as doubles (0 | 1), read-only.  get_open_boundary_stats: of the last renewal, over the faces of the open patches, the number of inflow faces, the sum of phi
 * over them (< 0) and over the outflow faces; any pointer may be NULL; FY_ERR_INVALID when no patch carries an open code.  Only this call waits for the device.  The
 * clock is "open_boundary" of fy_ldu_solver_get_kernel_timing (no launch without an open patch: nothing is allocated, every kernel takes the path it always took). */
int fy_ldu_solver_get_open_boundary_stats(fy_ldu_solver*, int64_t* inflow_faces, double* inflow_flux, double* outflow_flux);
/* Porous zones as on fy_solver (fy_solver_set_porous_zones): `cells` are cell labels of the fy_poly_mesh; the same refusals, read-outs ("porousZone", "mom_bd") and
 * the "porous_force" clock of fy_ldu_solver_get_kernel_timing */
int fy_ldu_solver_set_porous_zones(fy_ldu_solver*, const fy_porous_desc*);
int fy_ldu_solver_get_porous_stats(fy_ldu_solver*, int32_t* n_zones, int64_t* cells, double* volume, double* void_volume, double* force);
/* Heat exchange (fy_ldu_case.thermal.on; FY_ERR_INVALID on a solver without it): the entry points of fy_solver one for one, with the same semantics.  While thermal is
 * on, "T" [nc] (also writable: a non-uniform start), "heatSp" [nc] (W/K), "heatSu" [nc] (W) and, with thermal.beta != 0 and g != 0, "buoyancy" [nc][3] are field names
 * of fy_ldu_solver_read_field_host, and "T" one that fieldAverage accepts. */
int fy_ldu_solver_set_particle_temperatures_host(fy_ldu_solver*, int batch, const double* Tp);
int fy_ldu_solver_set_particle_temperatures_device(fy_ldu_solver*, int batch, const double* d_Tp);
int fy_ldu_solver_get_particle_heat_host(fy_ldu_solver*, int batch, double* q);
int fy_ldu_solver_get_thermal_stats(fy_ldu_solver*, int32_t* iterations, double* initial_residual, double* heat_to_particles_W);
int fy_ldu_solver_get_particle_thermal_state(fy_ldu_solver*, int batch, double* Tp, int64_t* resets);
int fy_ldu_solver_hold_sources(fy_ldu_solver*, int on);                    /* as fy_solver_hold_sources: setSourceZero deferred to the next step's start (runTime.write() sees alpha / uSource) */
/* Point-force mode (icoFoamYade): the cell mesh.findCell (FoamYade.C:251) gave each particle of the last fy_set_particles_* at the last step, in the caller's order,
 * -1 where fy_get_found_host says -1.  Read-only; waits for the device.  mesh.findCell is decided by OpenFOAM's face-fan tetrahedra (polyMesh::CELL_TETS; star-shaped
 * cells): a point on a shared triangle, edge or vertex gets one of the cells that share it.  In Gaussian mode (pimpleFoamYade) a particle has a stencil of cells, not
 * one cell: FY_ERR_UNSUPPORTED, fy_last_error() names this call (fy_get_stencils_host on fy_ldu_solver_coupling() gives the stencils).  FY_ERR_INVALID until a step
 * has located the particles last set (before the first step; between fy_set_particles_* and the next step). */
int fy_ldu_solver_get_particle_cells_host(fy_ldu_solver*, int32_t* out_cells /* [n] */);
fy_ctx* fy_ldu_solver_coupling(fy_ldu_solver*);                              /* FoamYade on this mesh (point force); fy_set_particles_* as usual */
/* fields by name, host copies: "U" [nc][3], "p", "phi" [n_faces], "uSource" [nc][3] (added to what the coupling leaves: an external momentum source),
 * "rAU", "HbyA", "phiHbyA", "p_diag", "p_coef" [n_faces], "p_rhs", "vGrad" [nc][9]; with pimpleFoamYade "alpha" [nc], "alphaf" [n_faces] (the void fraction on the faces, 1 on the boundary), "uSourceDrag", "uParticle"; with heat transfer "T", "heatSp", "heatSu", "buoyancy" (below); geometry: "C" "V" "Cf" "Sf" "magSf" "w" "dcNO" "kvec";
 * "nearWallDist" [n_faces - n_internal_faces]: y of each boundary face on a patch with a wall-function nut or epsilon (0 elsewhere) [OF-6 nearWallDist::correct];
 * "nut_boundary" [n_faces - n_internal_faces]: nut on each boundary face as the equations see it now (what the last correctNut() left; the file's value before) */
int fy_ldu_solver_field_count(fy_ldu_solver*, const char* name, int64_t* count);
int fy_ldu_solver_read_field_host(fy_ldu_solver*, const char* name, double* out);
int fy_ldu_solver_write_field_host(fy_ldu_solver*, const char* name, const double* in);
/* the pressure equation's operators as the last step left them, on host vectors of n_cells: "p_matrix" out = A in, "p_precondition" out = M^-1 in
 * (the V-cycle, or the diagonal) -- for tests of the solver's algebra (symmetry, definiteness, the cycle's contraction) */
int fy_ldu_solver_apply(fy_ldu_solver*, const char* op, const double* in, double* out);
/* the multigrid hierarchy of FY_PSOLVER_PCG_MG: cells and matrix slots (neighbours per row, padded) per level, finest first; n_levels = 0 without one */
int fy_ldu_solver_mg_levels(fy_ldu_solver*, int cap, int32_t* cells, int32_t* slots, int* n_levels);
/* one array of one level of that hierarchy, as doubles, copied from the device on the solver's stream (a diagnostic: nothing on the step's path reads it):
 * "diag" [cells] (level 0: the solver's p_diag), "coef" and "nbr" [slots * cells] slot-major (padding: the cell itself with coefficient 0, after the row's
 * entries), "agg" [cells]: this level's cell -> the next level's (count 0 on the last level), "inv" [cells * cells]: the last level's dense inverse (count 0
 * elsewhere).  out = NULL: only *count is set.  "diag", "coef", "inv" are those of the last pressure assembly (step first) */
int fy_ldu_solver_mg_level_read(fy_ldu_solver*, int level, const char* what, int64_t cap, double* out, int64_t* count);
int fy_ldu_solver_destroy(fy_ldu_solver*);

/* An OpenFOAM case directory whose constant/polyMesh is ANY mesh of wall / patch boundaries (ASCII), for icoFoamYade or (laminar, fixed time step)
 * pimpleFoamYade: what createMesh.H + createFields.H read (icoFoamYade.C:42-44, pimpleFoamYade.C:41-43).  The object is the fy_foam_case above with the mesh kept in OpenFOAM's addressing:
 * fy_foam_case_info_get, fy_foam_case_initial_fields, fy_foam_case_write_fields and fy_foam_case_close work on it; fy_foam_case_desc refuses it
 * (there is no block to describe).  fvSchemes must ask for what fy_ldu_solver does: Gauss linear, `corrected` laplacian / snGrad. */
int fy_foam_case_open_general(const char* case_dir, int solver /* FY_SOLVER_ICO | FY_SOLVER_PIMPLE */, fy_foam_case** out);
int fy_foam_case_poly_mesh(const fy_foam_case*, fy_poly_mesh* out);              /* pointers into the case object: valid until fy_foam_case_close */
int fy_foam_case_ldu_desc(const fy_foam_case*, fy_ldu_case* out);                 /* ready for fy_ldu_solver_create (patch arrays point into the case object) */
int fy_foam_case_patch_name(const fy_foam_case*, int patch, char* out, int cap); /* the boundary file's order = fy_poly_mesh's patch numbers */
int fy_foam_case_write_time_ldu(const fy_foam_case*, fy_ldu_solver*, const char* time_name);     /* runTime.write() (icoFoamYade.C:142): <time>/U, p; with flow control on also <time>/uniform/meanVelocityForceProperties */
int fy_foam_case_write_wall_loads_ldu(const fy_foam_case*, fy_ldu_solver*);                         /* fy_foam_case_write_wall_loads for a general case */
int fy_foam_case_write_monitors_ldu(const fy_foam_case*, fy_ldu_solver*);                           /* fy_foam_case_write_monitors for a general case */
int fy_foam_case_restore_averages_ldu(const fy_foam_case*, fy_ldu_solver*, int* restored);         /* fy_foam_case_restore_averages for a general case */

/* Porous zones of a case directory, block or general (one reader): the sub-dictionary of constant/couplingProperties
 *     porousZones { plate { type DarcyForchheimer; box (x0 y0 z0) (x1 y1 z1); d (dx dy dz); f (fx fy fz); } ... }
 * A cell belongs to a zone if its centre lies in the closed box (boxToCell's rule; the centres are the solver's); `active off;` is accepted and leaves the zone out.
 * Refused by name with what is accepted (FY_ERR_UNSUPPORTED): any other key (cellZone, coordinateSystem, selectionMode, ...), another type, a box that selects no
 * cell, boxes that share a cell, a negative or non-finite coefficient, more than FY_POROUS_MAX_ZONES active zones, a decomposed case.  A file without the
 * sub-dictionary gives no zones.  Nothing is written to a time directory: a restart reads the same file.
 * _porous_zones: the descriptor for fy_solver_set_porous_zones / fy_ldu_solver_set_porous_zones (the cell lists point into the case object: valid until
 * fy_foam_case_close).  _make_solver / _make_ldu_solver: fy_foam_case_desc + fy_solver_create (fy_foam_case_poly_mesh + fy_foam_case_ldu_desc +
 * fy_ldu_solver_create) and the case's zones applied -- the descriptors themselves carry no zones, so a solver created from them alone has none */
int fy_foam_case_porous_zones(const fy_foam_case*, fy_porous_desc* out);
int fy_foam_case_make_solver(const fy_foam_case*, const fy_transport*, int device_ordinal, fy_solver** out);
int fy_foam_case_make_ldu_solver(const fy_foam_case*, const fy_transport*, int device_ordinal, fy_ldu_solver** out);

#ifdef __cplusplus
}
#endif
#endif /* FOAMYADE_HIP_H */
