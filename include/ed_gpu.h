/*
 * ed_gpu.h — C-ABI of the MI355X-native Lanczos H·v hot path for dmft-ed.
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain
 * pointers and sizes, returns an int status (ED_OK = 0) and leaves a message in
 * ed_gpu_last_error() on failure.  Nothing here mentions torch or HIP types:
 * streams are passed as `void*` (a hipStream_t, or NULL for the default stream).
 *
 * Two layers:
 *   1. Reference-shaped global API (ed_gpu_init / ed_gpu_build_sector /
 *      ed_gpu_hxv / ed_gpu_delete_sector ...).  It keeps one "current sector",
 *      exactly like the module state Hsector/H/spH0 of the reference, so that a
 *      Fortran procedure pointer with the cc_sparse_HxV interface can call it
 *      unchanged (see dmft-ed_amd/fortran/ed_gpu_hxv.f90 and INTEGRATION.md).
 *   2. Handle API (ed_sector_*) used by the sector / Green's-function seed farm,
 *      where many sectors live at once on several GPUs.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   ed_params                 <- effective_bath (ED_VARS_GLOBAL.f90:12-22), impHloc
 *                                (ED_VARS_GLOBAL.f90:73), Uloc/Ust/Jh/Jx/Jp/xmu/hfmode
 *                                (ED_INPUT_VARS.f90:17-31), Jhflag (ED_SETUP.f90:289-290)
 *   ed_gpu_build_sector       <- build_Hv_sector        ED_HAMILTONIAN.f90:42-103
 *                                (+ build_sector ED_SETUP.f90:886-984,
 *                                   ed_buildH_c ED_HAMILTONIAN_STORED_HxV.f90:28-113)
 *   ed_gpu_hxv                <- cc_sparse_HxV          ED_VARS_GLOBAL.f90:48-54
 *                                = spMatVec_cc          ED_HAMILTONIAN_STORED_HxV.f90:132-143
 *                                / directMatVec_cc      ED_HAMILTONIAN_DIRECT_HxV.f90:21-92
 *   ed_gpu_delete_sector      <- delete_Hv_sector       ED_HAMILTONIAN.f90:106-123
 *                                (safe after a direct build, unlike the reference)
 *   ed_gpu_vecdim             <- vecDim_Hv_sector       ED_HAMILTONIAN.f90:126-149
 *   ed_gpu_dump_csr           <- sp_dump_matrix         ED_SPARSE_MATRIX.f90:331-388
 *                                (row-of-arrays order of sp_insert_element :249-320;
 *                                ed_gpu_nnz sizes its arrays)
 *   ed_gpu_lanc_eigh          <- sp_lanc_eigh (SciFortran; spec .repo/PLAIN_LANCZOS.f90:286-385)
 *   ed_gpu_lanc_tridiag       <- sp_lanc_tridiag (SciFortran; spec .repo/PLAIN_LANCZOS.f90:154-180)
 *   ed_gpu_eigh               <- sp_eigh (ARPACK; called at ED_DIAG.f90:145-167)
 *   ed_sector_nn_moments      <- observables_impurity   ED_OBSERVABLES.f90:48-715 and
 *   ed_sector_expect             local_energy_impurity  ED_OBSERVABLES.f90:726-980
 *                                (their sums over the kept vector's elements)
 *   ed_sector_twin_vector     <- es_return_cvector      ED_EIGENSPACE.f90:414-445 of a twin entry
 *                                (twin_sector_order / flip_state ED_SETUP.f90:1123-1186,
 *                                 get_twin_sector ED_SETUP.f90:1196-1212)
 *   ed_sector_seed_batch      <- the vvinit loops of lanc_build_gf_normal_c / _mix_c
 *                                ED_GF_NORMAL.f90:159-174, ED_GF_NORMAL.f90:312-344
 *   ed_sector_seed_plan       <- the six vvinit loops of lanc_build_gf_superc_c
 *                                ED_GF_SUPERC.f90:119-439
 *   ed_sector_seed_pair       <- the vvinit loops of the pair susceptibility
 *                                ED_GF_CHIPAIR.f90:98-102, ED_GF_CHIPAIR.f90:144-148 and of
 *                                lanc_ed_build_densChi_mix_c ED_GF_CHIDENS.f90:523-586,
 *                                ED_GF_CHIDENS.f90:596-659
 */
#ifndef ED_GPU_H
#define ED_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- limits */
#define ED_MAX_NORB  3   /* ed_checks_global: Norb<=3  (ED_SETUP.f90:56) */
#define ED_MAX_NSPIN 2   /* ed_checks_global: Nspin<=2 (ED_SETUP.f90:55) */
#define ED_MAX_NBATH 32
#define ED_MAX_NS    16  /* levels per spin: states are 2*Ns <= 32 bit words */

/* ---------------------------------------------------------------- enums */
#define ED_MODE_NORMAL 0 /* ed_mode='normal' : sectors (nup,ndw)        */
#define ED_MODE_SUPERC 1 /* ed_mode='superc' : sectors sz = nup-ndw     */
#define ED_MODE_NONSU2 2 /* ed_mode='nonsu2' : sectors n  = nup+ndw     */

#define ED_BATH_NORMAL  0 /* bath_type='normal'  */
#define ED_BATH_HYBRID  1 /* bath_type='hybrid'  */
#define ED_BATH_REPLICA 2 /* bath_type='replica' */

/* build flags (bit set) */
#define ED_STORED 0x1 /* ed_sparse_H=T: assemble H on the device (SELL-64 layout) */
#define ED_DIRECT 0x2 /* ed_sparse_H=F: matrix-free H·v, elements regenerated     */
#define ED_REAL   0x4 /* store H as real(8) (only when impHloc and bath are real) */
#define ED_NO_PACK   0x10 /* stored: plain SELL arrays only (no {col|value index} words) */
#define ED_KRON2_OFF 0x20 /* matrix-free Kronecker form: one-pass k_kron only       */
#define ED_KRON2_ON  0x40 /* two-pass Kronecker tables below the size threshold too */
#define ED_NO_SPLIT  0x80 /* stored: no two-segment form (one-pass k_spmv_pk only)          */
#define ED_SPLIT_ON  0x100 /* stored: two-segment form below the size threshold too        */
#define ED_FUSED_ON  0x200 /* stored: fused one-pass re-laid form below the size threshold too */
#define ED_NO_FUSED  0x400 /* stored: no fused one-pass re-laid form                       */

/* Kernel-selection options of a built sector (ed_sector_set_options): the
 * alternatives kept for parity tests and A/B measurements.  0 = the default
 * choice everywhere; nothing in the library reads the environment.  Bits
 * 0x010, 0x400, 0x8000 and 0x10000-0x80000 belonged to alternatives measured
 * slower and removed in round 5 (DESIGN.md keeps their numbers); they are
 * rejected as unknown. */
#define ED_OPT_NO_PERSIST     0x001 /* Lanczos: graph-captured multi-kernel recurrence only   */
#define ED_OPT_PERSIST_STORED 0x002 /* Lanczos: persistent MODE 0 (stored matrix from L2)      */
#define ED_OPT_NO_PREG        0x004 /* Lanczos: no register-resident modes (2, 3, 4)           */
#define ED_OPT_NO_PKRON       0x008 /* Lanczos: no Kronecker register layout (MODE 4)          */
#define ED_OPT_SPLIT_SIMPLE   0x020 /* kron_rows/cols: one-thread-per-row kernels              */
#define ED_OPT_NO_BATCH       0x040 /* lanc_tridiag_batch: seeds one after the other           */
#define ED_OPT_EIGH_NO_VERIFY 0x080 /* eigh: no deflated search for missed degenerate copies   */
#define ED_OPT_TRLAN_UNFUSED  0x100 /* eigh: four-sweep CGS2 instead of the fused sweeps       */
#define ED_OPT_TRLAN_NOFOLD   0x200 /* eigh: separate coefficient kernels on small grids       */
#define ED_OPT_NO_GRAPH       0x800 /* eigh: Krylov sweeps launched directly, not as hipGraphs  */
#define ED_OPT_TRLAN_NOLOCAL  0x1000 /* eigh: plain w = H v_j (no shifted three-term step)     */
#define ED_OPT_TRLAN_NOSOLO   0x2000 /* eigh: multi-kernel CGS also on sectors <= 2048 rows     */
#define ED_OPT_TRLAN_FULLUPD  0x4000 /* eigh: full CGS update every step (no local-only update) */
#define ED_OPT_STORED_EXACT 0x100000 /* stored H·v: the one-pass kernel (spMatVec_cc's per-row order,
                                        bit-identical) even where the two-segment form is built */
#define ED_OPT_NO_FUSED     0x400000 /* stored H·v: not the fused re-laid one-pass kernel (the
                                        two-segment form where built, else the one-pass one) */
#define ED_OPT_EIGH_NOHINT  0x800000 /* eigh: degeneracy screen from a pure hash start (no next
                                        Ritz vector mixed in) */
#define ED_OPT_EIGH_FULLPROBE 0x200000 /* eigh: no plain-Lanczos screen before the thick-restart
                                          degeneracy probe (every probe round runs it in full) */
#define ED_OPT_TWIN_GATHER 0x1000000 /* twin_vector into this sector (normal mode): the gather
                                        kernel of the other modes, not the tiled transpose */

/* status codes */
#define ED_OK              0
#define ED_ERR_ARG         1
#define ED_ERR_STATE       2
#define ED_ERR_HIP         3
#define ED_ERR_OOM         4
#define ED_ERR_UNSUPPORTED 5
#define ED_ERR_NOCONV      6 /* iterative solve did not converge */

/* ---------------------------------------------------------------- params
 * All arrays are C row-major over the MAXIMUM dimensions below; only the
 * leading [nspin][nspin][norb][norb][nbath] part is read.  Index i of a C array
 * here is Fortran index i+1 of the reference array.
 *   imphloc_*[ispin][jspin][iorb][jorb]      = impHloc(ispin+1,jspin+1,iorb+1,jorb+1)
 *   bath_e[ispin][iorb][k]                   = dmft_bath%e(ispin+1,iorb+1,k+1)
 *     (bath_type='hybrid': only iorb=0 is used, as size(e,2)=1)
 *   bath_v/u/d[ispin][iorb][k]               = dmft_bath%v/u/d(...)
 *   bath_h_*[ispin][jspin][iorb][jorb][k]    = dmft_bath%h(...)   (replica)
 *   bath_vr_*[k]                             = dmft_bath%vr(k+1)  (replica)
 */
typedef struct ed_params {
  int32_t norb, nspin, nbath;
  int32_t ed_mode;   /* ED_MODE_*  */
  int32_t bath_type; /* ED_BATH_*  */
  int32_t hfmode;    /* logical    */
  double uloc[3];
  double ust, jh, jx, jp, xmu;
  double imphloc_re[ED_MAX_NSPIN][ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NORB];
  double imphloc_im[ED_MAX_NSPIN][ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NORB];
  double bath_e[ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NBATH];
  double bath_v[ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NBATH];
  double bath_u[ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NBATH];
  double bath_d[ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NBATH];
  double bath_h_re[ED_MAX_NSPIN][ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NORB][ED_MAX_NBATH];
  double bath_h_im[ED_MAX_NSPIN][ED_MAX_NSPIN][ED_MAX_NORB][ED_MAX_NORB][ED_MAX_NBATH];
  double bath_vr_re[ED_MAX_NBATH];
  double bath_vr_im[ED_MAX_NBATH];
  /* Jz_basis (ED_INPUT_VARS.f90:78, nonsu2 only): sectors are (n, twoJz) with
   * twoJz = twoSz + twoLz, twoLz = sum over levels of 2*Lzdiag(iorb) with
   * Lzdiag = [-1,+1,0] (ED_VARS_GLOBAL.f90:207) and iorb-1 = level mod Norb
   * (build_sector ED_SETUP.f90:940-965); q1 = n, q2 = twoJz.  H must conserve
   * Jz (replica bath with an Lz-basis Hloc): ed_sector_create checks it. */
  int32_t jz_basis;
  int32_t pad_;
} ed_params;

typedef struct ed_sector_info {
  int64_t dim;      /* getDim(isector)                                  */
  int64_t nnz;      /* stored elements incl. diagonal (0 for direct)    */
  int64_t padded;   /* SELL-64 slots actually stored (>= nnz - dim)     */
  int32_t ns;       /* levels per spin                                  */
  int32_t mode;     /* ED_MODE_*                                        */
  int32_t q1, q2;   /* (nup,ndw) | (sz,0) | (n,0) | (n,twoJz)           */
  int32_t flags;    /* ED_STORED|ED_DIRECT|ED_REAL as built             */
  int32_t kron;     /* 1 if the direct path uses the (DimUp x DimDw) form */
  int64_t dimup, dimdw;   /* factor dimensions (normal mode), else 0    */
  int64_t device_bytes;   /* device memory held by the sector           */
  int32_t packed;   /* 1 if stored H·v reads 32-bit {col|value index} words */
  int32_t npdict;   /* distinct off-diagonal values (packed dictionary)  */
  int64_t row0, nrows;    /* rows held: [row0, row0+nrows) (whole: 0, dim) */
  int32_t split;    /* 1 if the two-segment stored form is built (default stored H·v) */
  int32_t pad_;
  int64_t split_far;          /* cross-block elements (segment B)            */
  int64_t split_far_uniform;  /* of which stored once per 64-row slice (U)   */
  int64_t split_bytes;        /* bytes one two-segment launch reads of the re-laid matrix:
                                 4 * (A words + L words) + 8 * U entries + A slice pointers */
  int64_t split_list_bytes;   /* + segment B's work list and slice table       */
  int32_t fused;    /* 1 if the fused one-pass re-laid form is built (default stored H·v) */
  int32_t pad2_;
  int64_t fused_far;          /* cross-block elements                         */
  int64_t fused_far_uniform;  /* of which stored once per 64-row unit (U)     */
  int64_t fused_bytes;        /* bytes one fused launch reads of the re-laid matrix:
                                 4 * (A words + L words) + 8 * U entries + 40 * units */
} ed_sector_info;

typedef struct ed_sector ed_sector; /* opaque */

/* ------------------------------------------------------------ handle API */
/* Build the sector basis and (ED_STORED) the Hamiltonian on `device`.
 * q1,q2: (nup,ndw) for normal, (sz,-) for superc, (n,-) for nonsu2.
 * stream: NULL — the sector creates (and destroys) a private non-blocking
 * stream for its build and its synchronous entry points (eigh, lanczos, ...);
 * non-NULL — that stream is used instead and stays the caller's (it must
 * outlive the sector; a farm worker passes its own stream to every sector it
 * solves).  Do not pass the legacy default stream: it serialises with every
 * other stream of the device. */
int ed_sector_create(const ed_params* p, int32_t q1, int32_t q2, int32_t flags,
                     int32_t device, void* stream, ed_sector** out);
/* The reference's MPI row split of one sector (build_Hv_sector with
 * MpiStatus, ED_HAMILTONIAN.f90:55-62; spMatVec_mpi_cc STORED_HxV.f90:147-197):
 * build only rows [row0, row0+nrows) of H (ED_STORED, or ED_DIRECT generic).
 * ed_sector_hxv_dev[_path] then takes the WHOLE sector vector v (the
 * Allgatherv result) and writes the nrows local entries of Hv; columns stay
 * global.  Lanczos/eigh/apply_op refuse such a sector (ED_ERR_UNSUPPORTED):
 * the distributed recurrence runs on the host side (edgpu.dist). */
int ed_sector_create_rows(const ed_params* p, int32_t q1, int32_t q2, int32_t flags, int64_t row0,
                          int64_t nrows, int32_t device, void* stream, ed_sector** out);
int ed_sector_destroy(ed_sector* s);
/* Select kernel alternatives (ED_OPT_* bit set, replaces the previous set). */
int ed_sector_set_options(ed_sector* s, int32_t opts);
int ed_sector_get_info(const ed_sector* s, ed_sector_info* info);

/* H·v on device pointers (async on `stream`).  vtype: 0 = real(8) vectors,
 * 1 = complex(8) interleaved vectors.  hv is overwritten (not accumulated),
 * as spMatVec_cc does (Hv=zero first, STORED_HxV.f90:137). */
int ed_sector_hxv_dev(ed_sector* s, int32_t vtype, const void* v, void* hv, void* stream);
/* Same, forcing the matrix-free kernel even on a stored sector (1) or the
 * stored kernel (0). -1 = default for the sector. */
int ed_sector_hxv_dev_path(ed_sector* s, int32_t path, int32_t vtype, const void* v,
                           void* hv, void* stream);
/* Columns the held rows refer to (the halo of a row-split sector,
 * ed_sector_create_rows): mask_dev[(dim+31)/32] (device, zeroed here) gets bit
 * c set for every column c of an off-diagonal element of the held rows.
 * Async on `stream`.  edgpu.dist exchanges only these entries of the vector
 * instead of the reference's whole-vector Allgatherv (STORED_HxV.f90:175-189). */
int ed_sector_col_mask(const ed_sector* s, uint32_t* mask_dev, void* stream);
/* Host-pointer H·v (synchronous, complex(8) vectors of length nloc = dim). */
int ed_sector_hxv(ed_sector* s, int32_t nloc, const double* v, double* hv);

/* H%map(1:dim): the Fock states of the sector in reference order (uint32). */
int ed_sector_map(const ed_sector* s, uint32_t* map_host);
/* Dump the stored H in reference row order (diagonal first, then off-diagonal
 * elements in insertion order).  rowptr[dim+1], cols[nnz] are 0-based;
 * vals is complex interleaved (2*nnz doubles).  Requires ED_STORED. */
int ed_sector_dump_csr(const ed_sector* s, int64_t* rowptr, int32_t* cols, double* vals);

/* Read-only view of the device SELL-64 arrays of a stored sector (for
 * inspection / kernel experiments).  Entry k of row r lives at
 * sptr[r/64] + 64*k + r%64; the diagonal is separate.  vals/diag are real(8)
 * when value_bytes == 8, complex(8) interleaved when 16. */
typedef struct ed_sell_view {
  int64_t dim, nslice, slots;
  int32_t value_bytes, pad;
  const void* diag;
  const int64_t* sptr;
  const int32_t* cols;
  const void* vals;
  const uint16_t* rowcnt;
} ed_sell_view;
int ed_sector_sell_view(const ed_sector* s, ed_sell_view* view);

/* Device-resident plain Lanczos (3-term recurrence, no reorthogonalisation).
 * v0: host start vector (vtype as above) of length dim, or NULL for the
 * deterministic default start vector.  Outputs on the host. */
int ed_sector_lanc_tridiag(ed_sector* s, int32_t vtype, const void* v0, int32_t nitermax,
                           double threshold, double* alfa, double* beta, int32_t* nlanc);
/* Ground state: returns egs (lowest Ritz value) and, if vect != NULL, the
 * normalised Ritz vector (host or device pointer, vtype).  ncheck as
 * lanczos_plain_c. */
int ed_sector_lanc_eigh(ed_sector* s, int32_t vtype, const void* v0, int32_t nitermax,
                        double threshold, int32_t ncheck, double* egs, void* vect,
                        int32_t* nlanc);
/* Diagnostic: the Lanczos recurrence a run with (vtype, path) would use —
 * persistent one-workgroup mode 0 (stored, L2), 1 (Kronecker tables in LDS),
 * 2 (stored matrix in registers), 3 (its matrix-free twin), 4 (Kronecker
 * register layout) or -1 (graph-captured multi-kernel), under the sector's
 * ED_OPT_* options. */
int ed_sector_lanc_mode(ed_sector* s, int32_t vtype, int32_t path);
/* Diagnostic: the launch form of that recurrence, i.e. the k_lanc_persist
 * instantiation a run with (vtype, path) would start under the sector's
 * ED_OPT_* options.  Read-only: it reports what ed_sector_lanc_mode derives
 * (and caches) and chooses nothing of its own.
 *   geom[0]  mode as ed_sector_lanc_mode (-1: multi-kernel; geom[1..4] = 0)
 *   geom[1]  threads of the workgroup (1024 for modes 0/1, 512 for 2/3/4)
 *   geom[2]  template RPT, the row slots per thread
 *   geom[3]  template width: ELL row width W (modes 2/3), hop-list width E
 *            (mode 4), 1 for modes 0/1
 *   geom[4]  dynamic LDS bytes of the launch
 *   geom[5]  1 when H is held as complex(8) (HC forms), 0 when as real(8)
 * vtype 0 on a complex H is ED_ERR_ARG, as for the Lanczos entry points. */
int ed_sector_lanc_geom(ed_sector* s, int32_t vtype, int32_t path, int32_t geom[6]);
/* Lowest `nev` eigenpairs by thick-restart Lanczos with full (CGS2)
 * reorthogonalisation, Krylov basis of `ncv` vectors resident in HBM: the
 * device replacement of SciFortran's ARPACK sp_eigh (ED_DIAG.f90:145-167,
 * which="SR", Nblock=ncv, Nitermax=maxit restarts, tol as ARPACK:
 * |r_i| <= tol*max(eps^(2/3),|theta_i|)).  v0: host start vector or NULL.
 * evals[nev] ascending; evecs (host or device pointer, dim x nev
 * column-major, vtype) or NULL.
 * nconv: converged pairs; nhv: H·v products used.  ncv <= 64. */
int ed_sector_eigh(ed_sector* s, int32_t vtype, int32_t nev, int32_t ncv, int32_t maxit, double tol,
                   const void* v0, double* evals, void* evecs, int32_t* nconv, int32_t* nhv);
/* ed_sector_eigh (real vectors) for n stored sectors at once, the same
 * algorithm and options per sector: sectors of up to 2,640 rows run their
 * restart cycles and degeneracy-screen chunks as one workgroup each in a
 * shared launch (one launch and one host round trip per cycle for all of
 * them); larger ones run in lockstep, every kernel of a Krylov step carrying
 * that step of all of them; sectors the batch cannot take or finish are
 * solved by ed_sector_eigh's path afterwards.  The farm's replacement of
 * ED_DIAG.f90:71-249's loop over the sectors' sp_eigh calls.  maxit[i]:
 * sector i's Nitermax; v0[i] (host, or NULL / v0 NULL: the default start),
 * evals[i*nev + k], evecs[i] (host or device, dim x nev, or NULL), nconv[i],
 * nhv[i]; *nbatched: sectors finished inside the batch (or NULL); flags:
 * ED_BATCH_NO_FALLBACK leaves the others to the caller (their nconv[i] = -1,
 * e.g. to solve them on several threads); stream: the launches' stream
 * (NULL: the first sector's). */
#define ED_BATCH_NO_FALLBACK 0x1
int ed_sectors_eigh_batch(ed_sector* const* secs, int32_t n, int32_t nev, int32_t ncv, const int32_t* maxit,
                          double tol, const double* const* v0, double* evals, void* const* evecs,
                          int32_t* nconv, int32_t* nhv, int32_t* nbatched, int32_t flags, void* stream);
/* Fixed-length Lanczos on device pointers for benchmarking: runs exactly
 * `niter` iterations (no convergence test) from device vector v0 and writes
 * alfa/beta (host).  Returns the elapsed device time in ms in *ms (or NULL). */
int ed_sector_lanc_run(ed_sector* s, int32_t vtype, const void* v0_dev, int32_t niter,
                       double* alfa, double* beta, float* ms, void* stream);

/* Within-sector multi-GPU H·v (replaces the reference's MPI
 * row split + Allgatherv, ED_HAMILTONIAN.f90:55-62, STORED_HxV.f90:147-197)
 * for sectors built with ED_DIRECT that have the Kronecker form (info.kron):
 * H = D + Hup(x)1 + 1(x)Hdw on the DimDw x DimUp view of v.
 *   kron_rows: y[r][:] = D[w0+r][:] .* x[r][:] + Hup x[r][:]      (r < nw)
 *              x, y: the nw x DimUp row block of down rows [w0, w0+nw)
 *   kron_cols: yz[:][c] (+)= Hdw z[:][c]                           (c < nu)
 *              z, yz: the DimDw x nu strip of up columns [u0, u0+nu),
 *              row-major (c fastest); accumulate = 1 adds into yz
 * H v = rows(x) + cols(strip(x)) regathered: two all-to-alls per H·v, whose
 * row blocks are already the strip layout (edgpu.dist).  Device pointers,
 * async on `stream`. */
int ed_sector_kron_rows(ed_sector* s, int32_t vtype, int64_t w0, int64_t nw, const void* x, void* y,
                        void* stream);
int ed_sector_kron_cols(ed_sector* s, int32_t vtype, int64_t u0, int64_t nu, const void* z, void* yz,
                        int32_t accumulate, void* stream);

/* Green's-function seed (ED_GF_NORMAL.f90:159-174 / :216-229):
 *   dst(j) = sg * src(m)  for every basis state m of `src` with the level
 *   free (op = 1, c^+) or occupied (op = 0, c), |j> = op_level |m>,
 *   sg the Jordan-Wigner sign of c / cdg (ED_SETUP.f90:1080-1106).
 * `level` is the 0-based bit (Fortran position - 1).  dst is zeroed first.
 * Device pointers, async on `stream`; both sectors on the same device. */
int ed_sector_apply_op(const ed_sector* src, const ed_sector* dst, int32_t op, int32_t level,
                       int32_t vtype, const void* src_vec, void* dst_vec, void* stream);
/* Accumulating form for the mixed nonSU2 seeds (ED_GF_NONSU2.f90:571-595,
 * 739-763): dst(j) += (coef_re + i coef_im) * sg * src(m); dst is NOT zeroed.
 * vtype must be 1 (complex) when coef_im != 0. */
int ed_sector_apply_op_acc(const ed_sector* src, const ed_sector* dst, int32_t op, int32_t level,
                           double coef_re, double coef_im, int32_t vtype, const void* src_vec,
                           void* dst_vec, void* stream);
/* Every Green's-function seed of one (source vector, operator type, target
 * sector) group in one pass: the vvinit loops ED_GF_NORMAL.f90:159-174 (one
 * term) and ED_GF_NORMAL.f90:312-344 (two terms) with their dot_product and
 * divide.  Seed q is
 *   sum_l coef[q][l] * op_{levels[l]} |src_vec>,  normalised;
 * norm2[q] = <seed|seed> before normalisation; a seed with norm2 == 0 is left
 * all zero.  levels: nlev distinct 0-based bits, nlev <= 2*ED_MAX_NORB, every
 * one reaching the same dst (ED_ERR_ARG otherwise, as ed_sector_apply_op);
 * coef: [nseed][nlev] (re, im) pairs, host, nseed <= 32, an imaginary part
 * needs vtype = 1; a coefficient (0, 0) leaves the level out of the seed.
 * Terms are added in level order: a coefficient 1 followed by coef * second
 * gives the unnormalised values of ed_sector_apply_op + ed_sector_apply_op_acc
 * bit for bit.  seeds: device, [nseed][dst->dim], written whole (no memset
 * needed).  The norms are summed in a fixed order: two calls on the same
 * input return the same bits.  Synchronous on `stream` (norm2 is a host
 * result).
 * The four ed_sector_seed_* entries share these checks, all made before
 * anything is launched, so a refused call leaves seeds and norm2 untouched:
 * ED_ERR_ARG unless the pointers are non-null, vtype is 0 or 1, the sectors
 * are on one device and of one model, and seeds does not overlap src_vec
 * (the kernels read src_vec while they store seeds); ED_ERR_UNSUPPORTED for
 * a row-split sector. */
int ed_sector_seed_batch(const ed_sector* src, const ed_sector* dst, int32_t op,
                         int32_t nlev, const int32_t* levels,
                         int32_t nseed, const double* coef,
                         int32_t vtype, const void* src_vec,
                         void* seeds, double* norm2, void* stream);
/* The same for a group whose images mix operator types: the superconducting
 * seeds of lanc_build_gf_superc_c, ED_GF_SUPERC.f90:119-166 (c^+_up),
 * ED_GF_SUPERC.f90:219-268 (c_dw) and ED_GF_SUPERC.f90:320-378 (their sum)
 * into sz+1, ED_GF_SUPERC.f90:168-217, ED_GF_SUPERC.f90:270-318 and
 * ED_GF_SUPERC.f90:380-439 into sz-1.  Image l is ops[l] (0: c, 1: c^+) on
 * the 0-based bit levels[l] of |src_vec>; seed s is image terms[2s], or image
 * terms[2s] + image terms[2s+1] (a negative second index: the first alone),
 * with unit coefficients, normalised; for a pair that is the arithmetic of
 * ed_sector_apply_op + ed_sector_apply_op_acc(coef = 1).  ED_ERR_ARG, before
 * anything is launched, unless 1 <= nlev <= 2*ED_MAX_NORB, 1 <= nseed <= 32,
 * every image maps src into dst (as ed_sector_apply_op), the (level, op) pairs
 * are distinct, every index is below nlev and the two of a seed differ.
 * seeds, norm2, determinism, the shared checks and synchronisation as
 * ed_sector_seed_batch. */
int ed_sector_seed_plan(const ed_sector* src, const ed_sector* dst,
                        int32_t nlev, const int32_t* levels, const int32_t* ops,
                        int32_t nseed, const int32_t* terms,
                        int32_t vtype, const void* src_vec,
                        void* seeds, double* norm2, void* stream);
/* Seeds of operators diagonal in the Fock basis, every one of a kept state in
 * one pass: the vvinit loops of the susceptibility builders
 * (ED_GF_CHISPIN.f90:98-103, ED_GF_CHISPIN.f90:194-199,
 * ED_GF_CHIDENS.f90:127-132) with their dot_product and divide.  Seed q is
 *   seeds[q][r] = (sum_l weight[q][l] * bit(map[r], levels[l])) * src_vec[r],
 * the sum in level order in double, then normalised; norm2[q] = <seed|seed>
 * before normalisation; a seed with norm2 == 0 is left all zero.  The seed
 * stays in the sector of src_vec: any whole sector, stored or direct, of any
 * ed_mode and of the Jz basis.  ED_ERR_ARG, before anything is launched,
 * unless 1 <= nlev <= 2*ED_MAX_NORB, the levels are distinct 0-based bits
 * below 2*Ns and 1 <= nseed <= 32.  weight: [nseed][nlev] real, host.  seeds:
 * device, [nseed][dim], written whole (no memset needed).  norm2,
 * determinism, the shared checks and synchronisation as
 * ed_sector_seed_batch. */
int ed_sector_seed_diag(const ed_sector* s, int32_t nlev, const int32_t* levels,
                        int32_t nseed, const double* weight,
                        int32_t vtype, const void* src_vec,
                        void* seeds, double* norm2, void* stream);
/* Seeds whose images are products of two ladder operators, every one of a
 * kept state and target sector in one pass: the vvinit loops of the pair
 * susceptibility, ED_GF_CHIPAIR.f90:98-102 (c_{a,dw} then c_{a,up}) and
 * ED_GF_CHIPAIR.f90:144-148 (c^+_{a,up} then c^+_{a,dw}), and of
 * lanc_ed_build_densChi_mix_c, ED_GF_CHIDENS.f90:523-586 (c^+_b c_a) and
 * ED_GF_CHIDENS.f90:596-659 (c^+_a c_b), with their dot_product and divide.
 * Image l is images[l] = (lev1, op1, lev2, op2): op2 (0: c, 1: c^+) on the
 * 0-based bit lev2 applied after op1 on lev1 to |src_vec>, lev1 != lev2; seed
 * s is image terms[2s], or image terms[2s] + image terms[2s+1] (a negative
 * second index: the first alone), with unit coefficients, normalised; that is
 * the arithmetic of ed_sector_apply_op into the intermediate sector followed
 * by ed_sector_apply_op_acc(coef = 1).  src == dst is allowed.  ED_ERR_ARG,
 * before anything is launched, unless 1 <= nimg <= 12, 1 <= nseed <= 12,
 * lev1 != lev2, every image maps src into dst exactly, no two images are the
 * same, every index is below nimg and the two of a seed differ.  seeds
 * ([nseed][dst->dim]), norm2, determinism, the shared checks and
 * synchronisation as ed_sector_seed_batch. */
int ed_sector_seed_pair(const ed_sector* src, const ed_sector* dst,
                        int32_t nimg, const int32_t* images,
                        int32_t nseed, const int32_t* terms,
                        int32_t vtype, const void* src_vec,
                        void* seeds, double* norm2, void* stream);
/* Vector of a twin entry of the state list (es_return_cvector,
 * ED_EIGENSPACE.f90:414-445; twin_sector_order and flip_state,
 * ED_SETUP.f90:1123-1186), from its partner's vector:
 *   dst_vec[i] = src_vec[Order(i)],  Order = argsort(flip_state(map_src)),
 * i.e. row i of dst holds state s and takes the value of src's row of
 * flip_state(s); no sign, no conjugation.  flip_state exchanges the two
 * Ns-bit halves (normal, superc) or complements all 2*Ns bits (nonsu2).
 * dst must be the twin of src (get_twin_sector, ED_SETUP.f90:1196-1212):
 * (q2, q1) in normal mode (q1 == q2: the map of the sector onto itself), -sz
 * in superc, 2*Ns - n in nonsu2.  ED_ERR_ARG, nothing launched: another
 * sector pair, sectors of different models or devices, Jz_basis sectors
 * (get_twin_sector knows none), src_vec == dst_vec.  Row-split sectors:
 * ED_ERR_UNSUPPORTED.  Normal mode runs an LDS-tiled transpose of src's
 * DimDw x DimUp view unless dst has ED_OPT_TWIN_GATHER; the other modes gather
 * through src's index tables.  Device pointers, async on `stream`; the model
 * is assumed to have the twin symmetry, as in the reference. */
int ed_sector_twin_vector(const ed_sector* src, const ed_sector* dst, int32_t vtype, const void* src_vec,
                          void* dst_vec, void* stream);
/* Observables of a kept state from its device-resident vector
 * (observables_impurity ED_OBSERVABLES.f90:48-715, local_energy_impurity
 * ED_OBSERVABLES.f90:726-980; no host copy of the vector, no bdecomp /
 * binary_search per element).
 *
 * Occupation pair moments — the diagonal loops ED_OBSERVABLES.f90:127-158 and
 * the density-density / Hartree sums ED_OBSERVABLES.f90:797-943 are linear in them:
 * M[p][q] = sum_i |v_i|^2 n_{levels[p]}(i) n_{levels[q]}(i), p <= q, packed row-major upper
 * triangle (nlev*(nlev+1)/2 doubles), followed by one more double: sum_i |v_i|^2.
 * nlev <= 2*ED_MAX_NORB.  Any whole sector (stored or direct).  out: host.  Synchronous on
 * stream (NULL: the sector's own). */
int ed_sector_nn_moments(const ed_sector* s, int32_t vtype, const void* vec_dev,
                         int32_t nlev, const int32_t* levels, double* out, void* stream);
/* Expectation values of operator strings — the off-diagonal sums
 * ED_OBSERVABLES.f90:556-581 (impurity density matrix), :631-654 (bath),
 * :802-846 (hopping energy), :882-927 (spin exchange, pair hopping) and the
 * magX / magY / phisc seeds :166-337 expanded:
 * out[t] = <v| T_t |v> = sum_i conj(v_{j(i)}) * sign * v_i  for nterm operator strings;
 * nops[t] in 1..4, levels/ops concatenated (op 0 = c, 1 = c^+; level the 0-based bit, as
 * ed_sector_apply_op), applied right to left.
 * out: 2*nterm doubles (re, im), host; vtype = 0 gives im = 0.  A term that leaves the
 * sector: ED_ERR_ARG, nothing launched.  Row-split sectors: ED_ERR_UNSUPPORTED. */
int ed_sector_expect(const ed_sector* s, int32_t vtype, const void* vec_dev, int32_t nterm,
                     const int32_t* nops, const int32_t* levels, const int32_t* ops,
                     double* out, void* stream);
/* sp_lanc_tridiag from a device start vector (not modified). */
/* v0_dev must be complete on entry (synchronise the stream that wrote it). */
int ed_sector_lanc_tridiag_dev(ed_sector* s, int32_t vtype, const void* v0_dev, int32_t nitermax,
                               double threshold, double* alfa, double* beta, int32_t* nlanc);
/* sp_lanc_tridiag for nseed device start vectors (v0_dev: nseed x dim,
 * contiguous, not modified) on the same sector — the Green's-function seeds
 * of one target sector (ED_GF_NORMAL.f90:180-193, ED_GF_NONSU2.f90:343-886).
 * Sectors that run the persistent one-workgroup recurrence take all seeds in
 * one launch, one workgroup per seed; alfa/beta/nlanc: nseed x nitermax /
 * nseed, each as ed_sector_lanc_tridiag. */
int ed_sector_lanc_tridiag_batch(ed_sector* s, int32_t vtype, int32_t nseed, const void* v0_dev,
                                 int32_t nitermax, double threshold, double* alfa, double* beta,
                                 int32_t* nlanc);
/* Stored H applied to nvec vectors in one pass over the matrix (spMatVec_cc,
 * STORED_HxV.f90:132-143, for every column): x_dev and y_dev are dim x nvec
 * blocks interleaved by row, element (row i, vector v) at i*nvec + v, of
 * real(8) (vtype 0) or complex(8) (vtype 1) values; nvec in {1, 2, 4, 8}.
 * Column v of y is bit-identical to ed_sector_hxv_dev of column v on a sector
 * with ED_OPT_STORED_EXACT.  Async on `stream`.  Refused before any launch,
 * nothing written: ED_ERR_ARG for nvec outside the set, a null pointer, y
 * overlapping x (x == y included), blocks not 16-byte aligned, vtype outside
 * {0, 1} or vtype 0 on a complex H; ED_ERR_UNSUPPORTED for a sector without a
 * stored matrix (ED_STORED) and for a row-split sector. */
int ed_sector_hxv_multi(ed_sector* s, int32_t vtype, int32_t nvec, const void* x_dev, void* y_dev,
                        void* stream);
/* sp_lanc_tridiag (.repo/PLAIN_LANCZOS.f90:87-118) for nseed device start
 * vectors advanced in lockstep: arguments and outputs as
 * ed_sector_lanc_tridiag_batch, any nseed >= 1.  The seeds are cut into groups
 * of 8, 4, 2, 1 whose vectors are interleaved by row; each Krylov step reads
 * the stored H once per group (ed_sector_hxv_multi's kernel) instead of once
 * per seed.  A seed that breaks down ends with its own nlanc while the others
 * of its group go on.  alfa and beta agree with the batch entry's to rounding
 * (the dot products are summed in another order), not bit for bit.  Refusals
 * as ed_sector_hxv_multi: the sector must be stored and whole. */
int ed_sector_lanc_tridiag_lockstep(ed_sector* s, int32_t vtype, int32_t nseed, const void* v0_dev,
                                    int32_t nitermax, double threshold, double* alfa, double* beta,
                                    int32_t* nlanc);
/* GF poles of one continued fraction (host, O(n^2)): E[n] ascending eigenvalues
 * of tridiag(alfa[0:n], beta[1:n]), z2[n] the squared first components of
 * their eigenvectors and (z1 != NULL) the first components themselves, Z(1,j).
 * Replaces tql2 in add_to_lanczos_gf_nonsu2 (ED_GF_NONSU2.f90:936;
 * ED_GF_SHARED.f90:76-214) and eigh in add_to_lanczos_gf_normal
 * (ED_GF_NORMAL.f90:612-618). */
int ed_tridiag_poles(int32_t n, const double* alfa, const double* beta, double* E, double* z2, double* z1);
/* Pole sums of nfrac continued fractions into device-resident G, in list
 * order — the inner loops of add_to_lanczos_gf_normal (ED_GF_NORMAL.f90:
 * 620-631) and add_to_lanczos_gf_nonsu2 (ED_GF_NONSU2.f90:936-950): fraction
 * f has npole[f] poles (E, z = Z(1,j): concatenated over fractions, host
 * arrays), weight pesoBZ = peso_bz[2f] + i peso_bz[2f+1], energy Ei[f], sign
 * isign[f] = +-1 and target component comp[f]; for every frequency
 *   gm[comp][i] += (pesoBZ*z_j)*z_j / (i*wm[i] - isign*(E_j - Ei))
 *   gr[comp][i] += (pesoBZ*z_j)*z_j / (wr[i] + i*eps - isign*(E_j - Ei))
 * pole by pole (the reference's addition order).  gm (ncomp x lmats), gr
 * (ncomp x lreal): complex(8) device arrays; wm[lmats], wr[lreal]: device.
 * Synchronous on `stream` (the host pole data is staged). */
int ed_gf_add_poles(int32_t nfrac, const int32_t* npole, const double* E, const double* z, const double* peso_bz,
                    const double* Ei, const int32_t* isign, const int32_t* comp, const double* wm, int32_t lmats,
                    const double* wr, int32_t lreal, double eps, double* gm, double* gr, void* stream);
/* Pole sums of nfrac tridiagonalisations into device-resident
 * susceptibilities, in list order: add_to_lanczos_spinChi
 * (ED_GF_CHISPIN.f90:254-323) called with isign = +1 and then -1.  Fraction f
 * has npole[f] poles (E, z = Z(1,j): concatenated, host), real weight peso[f]
 * (the state's weight times norm2), energy Ei[f] and target component
 * comp[f].  With D = E_j - Ei, p_j = (peso*z_j)*z_j and f_j = 1 - exp(-beta D)
 * = -expm1(-beta D):
 *   chi_iv[comp][0]  += 2 p_j s_j,   s_j = f_j / D, beta at D == 0
 *   chi_iv[comp][i]  += p_j f_j [1/(i vm[i] + D) - 1/(i vm[i] - D)],  i = 1..lmats
 *   chi_tau[comp][i] += p_j [exp(-tau[i] D) + exp(-(beta - tau[i]) D)],  i = 0..ltau
 *   chi_w[comp][i]   += p_j f_j [1/(wr[i] + i eps + D) - 1/(wr[i] + i eps - D)]
 * every -D term of a fraction pole by pole first, then every +D term (the
 * reference's addition order).  chi_iv (ncomp x (lmats+1)) and chi_w (ncomp x
 * lreal): complex(8) device arrays; chi_tau (ncomp x (ltau+1)): real(8);
 * vm[lmats+1], tau[ltau+1], wr[lreal]: device.  Synchronous on `stream`. */
int ed_chi_add_poles(int32_t nfrac, const int32_t* npole, const double* E, const double* z, const double* peso,
                     const double* Ei, const int32_t* comp, double beta, const double* vm, int32_t lmats,
                     const double* tau, int32_t ltau, const double* wr, int32_t lreal, double eps, double* chi_iv,
                     double* chi_tau, double* chi_w, void* stream);
/* The same with one isign call per fraction where asked: isign[f] = 0 is the
 * fraction of ed_chi_add_poles (+1 and then -1, the same additions in the same
 * order), +1 adds only the -D terms with the exp(-tau D) one and one s_j at
 * chi_iv[comp][0] (a seed O^+|n> of a non-Hermitian O), -1 only the +D terms
 * with exp(-(beta - tau) D) and one s_j (a seed O|n>).  isign == NULL: every
 * fraction takes both.  Any other value: ED_ERR_ARG, nothing is launched. */
int ed_chi_add_poles_signed(int32_t nfrac, const int32_t* npole, const double* E, const double* z,
                            const double* peso, const double* Ei, const int32_t* comp, const int32_t* isign,
                            double beta, const double* vm, int32_t lmats, const double* tau, int32_t ltau,
                            const double* wr, int32_t lreal, double eps, double* chi_iv, double* chi_tau,
                            double* chi_w, void* stream);

/* ------------------------------------------- self-energy and Weiss field
 * The second half of buildGF_impurity (ED_GREENS_FUNCTIONS.f90:22-63):
 * build_sigma_normal (ED_GF_NORMAL.f90:656-731), build_sigma_superc
 * (ED_GF_SUPERC.f90:826-929) and build_sigma_nonsu2 (from ED_GF_NONSU2.f90:977),
 * block by block.  One block: n impurity indices
 * idx[i] = ispin*norb + iorb, its one-body matrix h = impHloc - mu, and the
 * bath as np poles,
 *   Delta_ij(z) = sum_p c_p w[p][i] conj(w[p][j]) / (z - e[p]),
 *   invG0 = z - h - Delta,  G0 = invG0^-1,  Sigma = invG0 - G^-1.
 * nambu = 1: n = 2, idx[0] = idx[1] = iorb, the indices are (c_up, c+_dw) of
 * that orbital and G is read as [[G, F], [F, -conj(G)]], the last entry at the
 * mirrored index of a symmetric real grid. */
#define ED_SIGMA_MAX_N     6
#define ED_SIGMA_MAX_POLES 64
typedef struct ed_sigma_block {
  int32_t n, np, nambu, pad_;
  int32_t idx[ED_SIGMA_MAX_N];
  int32_t pad2_[2];
  double h[ED_SIGMA_MAX_N][ED_SIGMA_MAX_N][2];
  double e[ED_SIGMA_MAX_POLES];
  double c[ED_SIGMA_MAX_POLES][2];
  double w[ED_SIGMA_MAX_POLES][ED_SIGMA_MAX_N][2];
} ed_sigma_block;
/* The blocks and pole tables of p (host only, nothing is launched):
 * blocks[nspin*norb] at most, *nblk of them written.  ED_ERR_UNSUPPORTED for
 * superc with a hybrid or replica bath, whose orbital off-diagonal G and F are
 * not built. */
int ed_sigma_blocks(const ed_params* p, ed_sigma_block* blocks, int32_t* nblk);
/* Sigma, G0 and Delta of nblk blocks on the grids i w_n = i pi/beta (2n - 1),
 * n = 1..lmats, and w + i eps on the lreal points from wini to wfin, one work
 * item per (block, grid point) and one launch per distinct n.  gm, gr (and fm,
 * fr for Nambu blocks): complex(8) device arrays (nspin, nspin, norb, norb, L)
 * as build_gf leaves them; both NULL: only G0 and Delta are computed and
 * smats ... sareal are not touched.  Outputs: device arrays of the same
 * layout, zero outside the blocks; samats, sareal, f0mats, f0real only with
 * Nambu blocks.  ED_ERR_ARG, before anything is launched: n outside {1, 2, 3,
 * 4, 6}, np outside 1..64, two blocks sharing an index, a Nambu block on a
 * real grid with wini != -wfin, an output sharing a byte with an input or
 * another output.  Asynchronous on `stream`: no host synchronisation. */
int ed_sigma_build_blocks(int32_t nblk, const ed_sigma_block* blocks, int32_t nspin, int32_t norb, double beta,
                          int32_t lmats, double wini, double wfin, int32_t lreal, double eps, const double* gm,
                          const double* gr, const double* fm, const double* fr, double* smats, double* sreal,
                          double* g0mats, double* g0real, double* dmats, double* dreal, double* samats,
                          double* sareal, double* f0mats, double* f0real, void* stream);
/* The same with the blocks of ed_sigma_blocks(p). */
int ed_sigma_build(const ed_params* p, double beta, int32_t lmats, double wini, double wfin, int32_t lreal,
                   double eps, const double* gm, const double* gr, const double* fm, const double* fr, double* smats,
                   double* sreal, double* g0mats, double* g0real, double* dmats, double* dreal, double* samats,
                   double* sareal, double* f0mats, double* f0real, void* stream);

/* ------------------------------------------------------ reference-style API */
int ed_gpu_init(const ed_params* p);          /* ed_init_solver parameter hand-over */
int ed_gpu_set_device(int32_t device);
int ed_gpu_build_sector(int32_t q1, int32_t q2, int32_t flags, int64_t* dim);
int ed_gpu_vecdim(int32_t* vecdim);           /* vecDim_Hv_sector of the current sector */
/* cc_sparse_HxV(Nloc,v,Hv): Nloc by reference, complex(8) host arrays. */
int ed_gpu_hxv(const int32_t* nloc, const double* v, double* hv);
/* MPI variant of the current sector (MpiStatus=T in build_Hv_sector,
 * ED_HAMILTONIAN.f90:55-62, 85-101): this rank holds rows [row0, row0+nrows)
 * of H (nrows may be 0 when dim < MpiSize); vecDim_Hv_sector is then nrows. */
int ed_gpu_build_sector_rows(int32_t q1, int32_t q2, int32_t flags, int64_t row0, int64_t nrows,
                             int64_t* dim);
/* The reference's row split (ED_HAMILTONIAN.f90:55-62): MpiQ = dim/size, the
 * last rank also takes mod(dim,size); row0 = MpiIshift (0-based MpiIstart). */
int ed_gpu_mpi_split(int64_t dim, int32_t rank, int32_t size, int64_t* row0, int64_t* nrows);
/* spMatVec_mpi_cc (ED_HAMILTONIAN_STORED_HxV.f90:147-197) after its
 * MPI_Allgatherv: vin is the whole sector vector (dim, complex(8)), hv the
 * nloc = nrows local entries.  The Allgatherv itself stays in the caller's MPI
 * (the Fortran shim's gpuMatVec_mpi_cc).  Summation: every local row in the
 * reference's serial element order (spMatVec_cc); the reference's MPI kernel
 * adds the local-column elements first, so the two differ by rounding. */
int ed_gpu_hxv_mpi(const int32_t* nloc, const double* vin, double* hv);
/* Stored elements (diagonal included) of the rows the current sector holds:
 * the length a caller gives cols/vals of ed_gpu_dump_csr (rowptr: rows + 1).
 * ED_ERR_STATE without a current sector or on one built without ED_STORED. */
int ed_gpu_nnz(int64_t* nnz);
int ed_gpu_dump_csr(int64_t* rowptr, int32_t* cols, double* vals);
int ed_gpu_lanc_eigh(int32_t nitermax, double threshold, int32_t ncheck, double* egs,
                     double* vect, int32_t* nlanc);
/* sp_eigh(spHtimesV_cc, eig_values, eig_basis, Nblock, Nitermax, tol)
 * (ED_DIAG.f90:145-167, ARPACK which="SR"): device thick-restart Lanczos on
 * the current sector, complex(8) vectors.  v0 (dim, complex) or NULL;
 * evals[neigen] ascending; evecs complex(8) (dim x neigen, column-major) or
 * NULL; nconv converged pairs. */
int ed_gpu_eigh(int32_t neigen, int32_t nblock, int32_t nitermax, double tol, const double* v0,
                double* evals, double* evecs, int32_t* nconv);
int ed_gpu_lanc_tridiag(const double* v0, int32_t nitermax, double threshold,
                        double* alfa, double* beta, int32_t* nlanc);
int ed_gpu_delete_sector(void);
int ed_gpu_finalize(void);
const char* ed_gpu_last_error(void);
int ed_gpu_current_sector(ed_sector** out);   /* handle of the current sector */

#ifdef __cplusplus
}
#endif
#endif /* ED_GPU_H */
