// ed_eigh.hip — the thick-restart Lanczos eigensolver of a sector
// (ed_sector.hpp; kernels: ed_trlan.hpp), its degeneracy probe, the batched
// one-workgroup-per-sector solve (ed_trlbatch.hpp) and the lockstep
// multi-sector solve (ed_trlmulti.hpp), with their C-ABI entry points
// (include/ed_gpu.h).  Of the other units it calls launch_hxv (ed_hxv.hip).
#include "ed_sector.hpp"

#include <atomic>
#include <condition_variable>
#include <functional>
#include <thread>

#include "ed_trlan.hpp"
#include "ed_trlbatch.hpp"
#include "ed_trlmulti.hpp"
#include "ed_hosteig.hpp"

using namespace edg;

// (the host eigen-solvers and the restart / screen decisions: ed_hosteig.hpp)

__global__ void k_hash_vec(double* v, int64_t n, uint64_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    v[i] = hash_vec_unit(i, seed);
  }
}

// Thick-restart Lanczos state.  All O(dim) work and the CGS2 coefficients
// stay on the device; one expansion sweep (j0 .. m-1) is captured once per
// start column into a hipGraph (j0 = 0 and j0 = nkeep), so a restart cycle is
// one graph launch + one host sync for the m x m projected problem.
template <bool VC>
struct Trlan {
  using V = val_t<VC>;
  ed_sector* s = nullptr;
  int path = 0;
  hipStream_t st = nullptr;
  int64_t dim = 0;
  int G = 1, m = 0, mcap = 0;  // mcap: basis columns allocated
  bool fused = true;  // false (ED_OPT_TRLAN_UNFUSED): the four-sweep CGS2 (A/B)
  V *Vb = nullptr, *Xb = nullptr, *w = nullptr;
  double2 *h = nullptr, *coef = nullptr, *part = nullptr, *part2 = nullptr;
  // grids up to this fold the coefficient reduction into the next CGS pass
  // (every block re-reads G x ncol partials; 0 with ED_OPT_TRLAN_NOFOLD: A/B)
  // (round 6, in the 8-worker farm: folding at 256 or 512 blocks, with the
  // sweep grid at 512 or 256, within noise of 128, gpurun_out r6k; at the
  // closing build 256 with the 256-block grid: see kTrlanGridCap)
  int kFinFoldG = 256;
  bool graphs_on = true;  // false (ED_OPT_NO_GRAPH): sweeps launched directly
  bool solo = true;       // false (ED_OPT_TRLAN_NOSOLO): multi-kernel CGS on small sectors too (A/B)
  bool locupd = true;     // false (ED_OPT_TRLAN_FULLUPD): full CGS update every step (A/B)
  int* lof = nullptr;     // device: the current step's update was local-only
  double *Y = nullptr, *npart = nullptr, *alpha = nullptr, *beta = nullptr;
  double *npA = nullptr, *npB = nullptr;  // |w|^2 partials before / after the first CGS pass (DGKS)
  double* hp = nullptr;          // pinned staging (TrlStage)
  std::vector<void*> mine;
  std::vector<std::pair<int, hipGraphExec_t>> graphs;
  int nhv = 0;
  ~Trlan() {
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
    for (void* p : mine) (void)hipFreeAsync(p, st);
  }
  int alloc(void** p, size_t n) {
    HIPCK(hipMallocAsync(p, n, st));
    mine.push_back(*p);
    return ED_OK;
  }
  V* col(V* b, int c) { return b + (int64_t)c * dim; }
  // x -= V[:, :ncol] V[:, :ncol]^H x, twice; coef = summed coefficients;
  // with jn >= 0: alpha[jn], beta[jn] = ||x|| afterwards
  // one fused sweep (k_cgs) with the column group rounded up to 8/16/24/32
  bool cgs(int ncol, const double2* hin, V* x, double2* pt, double* np, const double2* pin = nullptr,
           int add = 0, const double* dgA = nullptr, const double* dgB = nullptr, int* lf = nullptr,
           const double* locA = nullptr) {
    const int nc = (ncol + 7) / 8 * 8;
#define ED_CGS(NCV) \
  hipLaunchKernelGGL((k_cgs<VC, NCV>), dim3(G), dim3(kBlock), 0, st, Vb, ncol, hin, x, dim, pt, np, pin, G, \
                     coef, add, dgA, dgB, lf, locA)
    if (nc <= 8) ED_CGS(8);
    else if (nc <= 16) ED_CGS(16);
    else if (nc <= 24) ED_CGS(24);
    else if (!VC && nc <= 32) ED_CGS(32);
    else return false;
#undef ED_CGS
    return true;
  }
  // jc: the basis column of v_j when it is not column jn (probe_screen's
  // rolling window; alpha/beta slot jn)
  int orth(int ncol, V* x, int jn, V* out = nullptr, int shifted = 0, int jc = -1) {
    // small sectors: the whole CGS2 + alpha/beta + V_{j+1} in one workgroup
    // (complex vectors: up to 16 columns; the 24/32-column forms spill)
    if (fused && solo && ncol > 0 && dim <= kOrthSoloMaxDim && ncol <= (VC ? 16 : 32)) {
      V* const o = (out && jn >= 0) ? out : nullptr;
      const int js = jn >= 0 ? jn : m;  // beta[m]: scratch slot
      const int nc = (ncol + 7) / 8 * 8;
#define ED_OSOLO(NCV)                                                                                          \
  hipLaunchKernelGGL((k_orth_solo<VC, NCV>), dim3(1), dim3(kOrthSoloBlock), 0, st, Vb, ncol, x, dim, coef,     \
                     jn >= 0 ? alpha : nullptr, beta, jn, js, o, shifted, (shifted && locupd) ? 1 : 0, jc)
      if (nc <= 8) ED_OSOLO(8);
      else if (nc <= 16) ED_OSOLO(16);
      else if constexpr (!VC) {
        if (nc <= 24) ED_OSOLO(24);
        else ED_OSOLO(32);
      }
#undef ED_OSOLO
      return ED_OK;
    }
    // fused CGS: dots + |x|^2 | x -= V h1, dots, |x'|^2 | (DGKS: only if
    // |x'| <= 0.717 |x|) x -= V h2, |x''|^2 — V streamed 2x or 3x
    if (fused && ncol > 0 && cgs(ncol, nullptr, x, part, npA)) {
      // shifted steps: the update may be local-only (cgs_loc_only, decided
      // by the first update pass from the dots and recorded in *lof)
      int* const lf = (shifted && locupd) ? lof : nullptr;
      const double* const la = lf ? npA : nullptr;
      if (G <= kFinFoldG) {
        // small grids: each pass forms the previous pass's coefficients from
        // its partials (k_vdot_fin folded in: 5 launches per step, not 7)
        cgs(ncol, nullptr, x, part2, npB, part, 0, nullptr, nullptr, lf, la);
        cgs(ncol, nullptr, x, nullptr, npart, part2, 1, npA, npB, lf);
      } else {
        hipLaunchKernelGGL(k_vdot_fin<VC>, dim3(ncol), dim3(kBlock), 0, st, part, G, h, coef, 0,
                           (const double*)nullptr, (const double*)nullptr);
        cgs(ncol, h, x, part2, npB, nullptr, 0, nullptr, nullptr, lf, la);
        hipLaunchKernelGGL(k_vdot_fin<VC>, dim3(ncol), dim3(kBlock), 0, st, part2, G, h, coef, 1,
                           (const double*)npA, (const double*)npB);
        cgs(ncol, h, x, nullptr, npart, nullptr, 0, npA, npB, lf);
      }
      if (out && jn >= 0)  // + V_{j+1} = x / beta_j in the same launch
        hipLaunchKernelGGL(k_coef_scale<VC>, dim3(G), dim3(kBlock), 0, st, npart, G, coef, jn, alpha, beta,
                           x, out, dim, shifted, jc);
      else
        hipLaunchKernelGGL(k_trl_coef, dim3(1), dim3(kBlock), 0, st, npart, G, coef, jn >= 0 ? jn : m,
                           jn >= 0 ? alpha : nullptr, beta, jn >= 0 ? shifted : 0, jc);
      return ED_OK;
    }
    if (ncol == 0) {
      hipLaunchKernelGGL(k_vaxpy<VC>, dim3(G), dim3(kBlock), 0, st, Vb, 0, h, x, dim, npart);
    }
    const dim3 gp(G, (ncol + kVCols - 1) / kVCols);
    for (int pass = 0; pass < 2 && ncol > 0; pass++) {
      hipLaunchKernelGGL(k_vdot_part<VC>, gp, dim3(kBlock), 0, st, Vb, ncol, x, dim, part);
      hipLaunchKernelGGL(k_vdot_fin<VC>, dim3(ncol), dim3(kBlock), 0, st, part, G, h, coef, pass,
                         (const double*)nullptr, (const double*)nullptr);
      hipLaunchKernelGGL(k_vaxpy<VC>, dim3(G), dim3(kBlock), 0, st, Vb, ncol, h, x, dim,
                         pass == 1 ? npart : nullptr);
    }
    hipLaunchKernelGGL(k_trl_coef, dim3(1), dim3(kBlock), 0, st, npart, G, coef, jn >= 0 ? jn : m,
                       jn >= 0 ? alpha : nullptr, beta, jn >= 0 ? shifted : 0, jc);  // beta[m]: scratch slot
    if (out && jn >= 0)
      hipLaunchKernelGGL(k_scale_into<VC>, dim3(grid_for(dim)), dim3(kBlock), 0, st, x, out, beta + jn, dim);
    return ED_OK;
  }
  // V[:, k0:k0+nout] = V[:, k0:k0+ncol] Y (Y on the device, ld ncol): in
  // place up to 32 columns, else through Xb and a copy back
  int rotate(int k0, int ncol, int nout, int g) {
    const dim3 gr(std::min(g, 2048));
    if (ncol <= 16)
      hipLaunchKernelGGL((k_rotate_ip<VC, 16>), gr, dim3(kBlock), 0, st, col(Vb, k0), ncol, Y, ncol, nout, dim);
    else if (ncol <= 32 && (!VC || ncol <= 24))
      hipLaunchKernelGGL((k_rotate_ip<VC, VC ? 24 : 32>), gr, dim3(kBlock), 0, st, col(Vb, k0), ncol, Y, ncol,
                         nout, dim);
    else {
      if (!Xb) CK(alloc((void**)&Xb, (size_t)mcap * dim * sizeof(V)));  // first use (nout < mcap)
      hipLaunchKernelGGL(k_rotate<VC>, gr, dim3(kBlock), (size_t)ncol * nout * sizeof(double), st, col(Vb, k0),
                         ncol, Y, ncol, nout, Xb, dim);
      HIPCK(hipMemcpyAsync(col(Vb, k0), Xb, (size_t)nout * dim * sizeof(V), hipMemcpyDeviceToDevice, st));
    }
    HIPCK(hipGetLastError());
    return ED_OK;
  }
  // Lanczos step j: w = H V_j, CGS2, alpha_j, beta_j; V_{j+1} = w / beta_j.
  // Past the sweep's first column (j > j0) the H·v applies the shifted
  // three-term recurrence (EpiTrlLoc) so that the DGKS test can skip the
  // second Gram-Schmidt pass; the first column after a restart couples to
  // every kept Ritz vector and takes the plain product.
  bool local = true;  // false (ED_OPT_TRLAN_NOLOCAL): plain w = H V_j every step (A/B)
  int step(int j, int j0) {
    nhv++;
    const bool loc = local && j > j0;
    // small packed stored sectors, real vectors: the whole step in one workgroup
    if constexpr (!VC) {
      if (solo && fused && path == 0 && s->d_words && !s->hc && s->row0 == 0 && s->nrows == dim &&
          dim <= kOrthSoloMaxDim && j + 1 <= 32) {
        StepSoloArgs a;
        a.diag = (const double*)s->d_diag;
        a.sptr = s->d_sptr;
        a.words = s->d_words;
        a.dict = (const double*)s->d_pdict;
        a.Vb = (const double*)Vb;
        a.x = (double*)w;
        a.out = j + 1 < m ? (double*)col(Vb, j + 1) : nullptr;
        a.coef = coef;
        a.alpha = alpha;
        a.beta = beta;
        a.dim = dim;
        a.j = j;
        a.shifted = loc ? 1 : 0;
        a.locupd = locupd ? 1 : 0;
        const int nc = (j + 1 + 7) / 8 * 8;
        if (nc <= 8) hipLaunchKernelGGL(k_step_solo<8>, dim3(1), dim3(kOrthSoloBlock), 0, st, a);
        else if (nc <= 16) hipLaunchKernelGGL(k_step_solo<16>, dim3(1), dim3(kOrthSoloBlock), 0, st, a);
        else if (nc <= 24) hipLaunchKernelGGL(k_step_solo<24>, dim3(1), dim3(kOrthSoloBlock), 0, st, a);
        else hipLaunchKernelGGL(k_step_solo<32>, dim3(1), dim3(kOrthSoloBlock), 0, st, a);
        HIPCK(hipGetLastError());
        return ED_OK;
      }
    }
    if (loc) {
      EpiTrlLoc<VC> e{w, col(Vb, j - 1), alpha + (j - 1), beta + (j - 1)};
      CK(launch_hxv<VC>(s, path, col(Vb, j), e, st));
    } else {
      EpiStore<VC> e{w};
      CK(launch_hxv<VC>(s, path, col(Vb, j), e, st));
    }
    CK(orth(j + 1, w, j, j + 1 < m ? col(Vb, j + 1) : nullptr, loc ? 1 : 0));
    return ED_OK;
  }
  int sweep(int j0) {
    const int n = m - j0;
    hipGraphExec_t ge = nullptr;
    for (auto& g : graphs)
      if (g.first == j0) ge = g.second;
    if (!ge && n > 2 && graphs_on) {
      hipGraph_t g;
      HIPCK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      int rc = ED_OK;
      for (int j = j0; j < m && rc == ED_OK; j++) rc = step(j, j0);
      hipError_t e2 = hipStreamEndCapture(st, &g);
      if (rc != ED_OK) return rc;
      HIPCK(e2);
      HIPCK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
      (void)hipGraphDestroy(g);
      graphs.emplace_back(j0, ge);
      nhv -= n;  // capture does not run anything
    }
    if (ge) {
      HIPCK(hipGraphLaunch(ge, st));
      nhv += n;
    } else {
      for (int j = j0; j < m; j++) CK(step(j, j0));
    }
    HIPCK(hipGetLastError());
    return ED_OK;
  }
};

// Pinned staging of one thick-restart solve (trlan_run's PinnedLease), offsets
// in doubles: alpha/beta down, the projected eigenvectors up (pageable copies
// go through the runtime's staging buffer, a CPU copy and an extra wait each,
// three per restart).  The device alpha | beta blocks have the same spacing.
struct TrlStage {
  static constexpr int kAlpha = 0, kBeta = kTrlanMaxCols + 8, kZ = 2 * kBeta;  // Z: up to 64 x 64
  static constexpr int kScalar = kZ + kTrlanMaxCols * kTrlanMaxCols + 8, kDoubles = kScalar + 8;
};

// blocks of the O(dim) Krylov sweeps
// (1024 until round 4: 512 measured 13 % faster per large-sector solve,
// tools/trlan_ab.py --grid; round 6 in the 8-worker farm: 128 and 256 within
// noise of 512, gpurun_out r6j; at the closing build — the medium sectors in
// the lockstep batch, the local-only CGS pass — 256 with the coefficient
// fold at 256 blocks (5 launches per step instead of 7): farm median 0.618
// -> 0.567 s over 6 reps each, lone (6,6) 82-84 -> 85 us per step, 128:
// 0.588 s, gpurun_out r6gc, profiles/r6/grid_cap_ab.json)
static constexpr int kTrlanGridCap = 256;
// ... except the largest sectors (configs[3]'s nine of 627,264-853,776 rows),
// whose lone solve is the critical path of a many-GPU farm: 512 blocks, the
// coefficient sums in their own launches (lone (6,6) 86.5-87.3 -> 83.6-84.2
// us per step, farm median 0.578 -> 0.570 s, gpurun_out r6big,
// profiles/r6/grid_big_ab.json)
static constexpr int64_t kTrlanBigDim = 600000;
// One thick-restart Lanczos solve on the columns [k0, m) of the basis; the
// columns [0, k0) are locked (deflation: every new vector is orthogonalised
// against them, their coefficients are not part of the projected matrix).
// Start vector: v0 (host) if given, else a hash vector from `seed`.  Returns
// the ma = m - k0 Ritz values (ascending) and the ma x ma rotation Z.
template <bool VC>
static int trlan_core(Trlan<VC>& T, int k0, int nev, int maxit, double tol, const void* v0, uint64_t seed,
                      std::vector<double>& theta, std::vector<double>& Z, int* conv_out) {
  using V = val_t<VC>;
  const int m = T.m, ma = m - k0;
  const int64_t dim = T.dim;
  hipStream_t st = T.st;
  const int g = grid_for(dim);
  const int64_t nd = dim * (VC ? 2 : 1);
  const size_t vs = sizeof(V);
  // V_k0 = v0 / |v0| (orthogonal to the locked columns)
  if (v0) HIPCK(hipMemcpyAsync(T.w, v0, dim * vs, hipMemcpyHostToDevice, st));
  else if (seed == 0) launch_default_start((double*)T.w, nd, st);
  else hipLaunchKernelGGL(k_hash_vec, dim3(grid_for(nd)), dim3(kBlock), 0, st, (double*)T.w, nd, seed);
  CK(T.orth(k0, T.w, -1));  // CGS2 against the locked columns; the norm -> beta[m]
  double* const hal = T.hp + TrlStage::kAlpha;
  double* const hbe = T.hp + TrlStage::kBeta;
  double* const hZ = T.hp + TrlStage::kZ;
  double* const hs = T.hp + TrlStage::kScalar;
  HIPCK(hipMemcpyAsync(hs, T.beta + m, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  const double b0 = hs[0];
  if (!(b0 > 0.0)) return fail(ED_ERR_ARG, "zero start vector");
  hipLaunchKernelGGL(k_scale_into<VC>, dim3(g), dim3(kBlock), 0, st, T.w, T.col(T.Vb, k0), T.beta + m, dim);

  std::vector<double> Tm((size_t)ma * ma, 0.0);
  int jstart = k0, conv = 0;
  uint64_t rseed = seed * 7919 + 1;
  for (int it = 0; it < maxit; it++) {
    int j0 = jstart;
    for (;;) {  // expansion j0..m-1, restarted past an invariant subspace
      CK(T.sweep(j0));
      // alpha | beta: one block on the device, laid out as the staging
      HIPCK(hipMemcpyAsync(hal, T.alpha, (TrlStage::kBeta + m) * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      const int jb = trl_fill(Tm.data(), ma, k0, j0, m, hal, hbe);
      if (jb < 0) break;
      // invariant subspace at jb: continue from a random direction orthogonal to V
      const int lb = jb - k0;
      Tm[lb + (size_t)ma * (lb + 1)] = Tm[(lb + 1) + (size_t)ma * lb] = 0.0;
      hipLaunchKernelGGL(k_hash_vec, dim3(grid_for(nd)), dim3(kBlock), 0, st, (double*)T.w, nd, rseed++);
      CK(T.orth(jb + 1, T.w, -1));
      hipLaunchKernelGGL(k_scale_into<VC>, dim3(g), dim3(kBlock), 0, st, T.w, T.col(T.Vb, jb + 1),
                         T.beta + m, dim);
      HIPCK(hipGetLastError());
      j0 = jb + 1;
      if (j0 >= m) break;
    }
    const double beta = hbe[m - 1];
    sym_eigh(ma, Tm, theta, Z);
    conv = trl_nconv(ma, nev, beta, theta.data(), Z.data(), tol);
    if (conv == nev || it == maxit - 1 || m == dim) break;
    const int nkeep = trl_nkeep(ma, nev);
    // (the previous restart's upload of hZ completed at this sweep's sync)
    std::copy(Z.begin(), Z.begin() + (size_t)ma * ma, hZ);
    HIPCK(hipMemcpyAsync(T.Y, hZ, (size_t)ma * ma * sizeof(double), hipMemcpyHostToDevice, st));
    CK(T.rotate(k0, ma, nkeep, g));
    hipLaunchKernelGGL(k_scale_into<VC>, dim3(g), dim3(kBlock), 0, st, T.w, T.col(T.Vb, k0 + nkeep),
                       T.beta + (m - 1), dim);
    HIPCK(hipGetLastError());
    trl_arrowhead(Tm.data(), ma, nkeep, beta, theta.data(), Z.data());
    jstart = k0 + nkeep;
  }
  *conv_out = conv;
  return ED_OK;
}

// Screening solve of the degeneracy probe (trlan_run): is there an
// eigenvalue of H below `cut` on the orthogonal complement of the locked
// columns [0, k0)?  A plain Lanczos recurrence from a hash start vector,
// without restarts and without keeping the Krylov basis: a rolling window of
// two columns (k0, k0+1) behind the locked ones holds v_{k-1} and v_k, and
// every step is orthogonalised against the locked columns and the window by
// the fused CGS (local-only when the locked coefficients are noise) — so a
// step streams k0 + 2 columns, not the k0 + 20 of the thick-restart probe,
// and the Krylov dimension is not capped by a restart.  Every kScreenChunk
// steps the host forms the lowest Ritz value theta of the tridiagonal and
// its residual bound |beta_k s_k| (first-row QL of the reversed matrix,
// tridiag_poles).  *below = 1: theta < cut — a certificate, since every
// Ritz value is a Rayleigh quotient and so >= the complement's lowest
// eigenvalue (the thick-restart probe then finds its vector); 0: theta
// converged to `tol` AND its whole residual interval [theta - r, theta + r]
// above the cut (none); -1: undecided within maxsteps (thick-restart probe).
// Round 5 also decided "none" on the interval alone after 30 steps; that only
// places the eigenvalue nearest theta, not the complement's lowest (an
// unconverged Ritz vector can carry little of a lower eigenvector), so round 6
// requires both.  The interval test matters on its own too: a missed copy just
// under the cut next to a well-converged theta just above it (r ~ tol|theta|
// > theta - lambda_min) fails the interval test and the run goes on until
// theta itself drops below the cut (tests/test_gpu_eigh.py adversarial case).
// The rules themselves: screen_decide (ed_hosteig.hpp).
// hint: column k0 holds the next Ritz vector of the main solve (round 0 of
// the probe) — the start vector is then the hash vector plus that Ritz
// vector at equal norm.  Where nothing was missed the complement's lowest
// eigenvector is the next one, which the mixed start already carries with
// weight ~1/2, so theta converges in fewer steps; a missed copy lies outside
// the main solve's Krylov space (in exact arithmetic) and is reached through
// the hash part, whose overlap with it is 1/sqrt(2) of a pure hash start's.
template <bool VC>
static int probe_screen(Trlan<VC>& T, int k0, int maxsteps, double tol, double cut, uint64_t seed, int* below,
                        bool hint = false) {
  using V = val_t<VC>;
  const int64_t dim = T.dim;
  hipStream_t st = T.st;
  const int64_t nd = dim * (VC ? 2 : 1);
  const int ca = k0, cb = k0 + 1;
  *below = -1;
  if (maxsteps < 2 || k0 + 2 > T.mcap) return ED_OK;
  // the recurrence's alpha/beta in T.alpha/T.beta's place for the duration
  double *pa = nullptr, *pb = nullptr;
  const int na = std::max(maxsteps, T.m) + 2;
  CK(T.alloc((void**)&pa, na * sizeof(double)));
  CK(T.alloc((void**)&pb, na * sizeof(double)));
  double* const sa = T.alpha;
  double* const sb = T.beta;
  struct Restore {
    Trlan<VC>& t; double* a; double* b;
    ~Restore() { t.alpha = a; t.beta = b; }
  } restore{T, sa, sb};
  T.alpha = pa;
  T.beta = pb;
  HIPCK(hipMemsetAsync(T.col(T.Vb, cb), 0, dim * sizeof(V), st));  // v_{-1} = 0
  hipLaunchKernelGGL(k_hash_vec, dim3(grid_for(nd)), dim3(kBlock), 0, st, (double*)T.w, nd, seed);
  if (hint)  // |hash|^2 ~ nd / 3 (uniform in [-1, 1)); the Ritz vector has unit norm
    hipLaunchKernelGGL(k_mix_hint, dim3(grid_for(nd)), dim3(kBlock), 0, st, (double*)T.w,
                       (const double*)T.col(T.Vb, ca), nd, sqrt((double)nd / 3.0));
  CK(T.orth(k0, T.w, -1));  // against the locked columns; the norm -> beta[m]
  hipLaunchKernelGGL(k_scale_into<VC>, dim3(grid_for(dim)), dim3(kBlock), 0, st, T.w, T.col(T.Vb, ca),
                     T.beta + T.m, dim);
  HIPCK(hipGetLastError());
  double* const hal = T.hp + TrlStage::kAlpha;  // alpha | beta of one chunk
  double* const hbe = T.hp + TrlStage::kBeta;
  std::vector<double> al, be;
  for (int k0s = 0; k0s < maxsteps; k0s += kScreenChunk) {
    const int k1 = std::min(maxsteps, k0s + kScreenChunk);
    for (int k = k0s; k < k1; k++) {
      const int cur = (k & 1) ? cb : ca, prv = (k & 1) ? ca : cb;
      T.nhv++;
      if (k == 0) {
        EpiStore<VC> e{T.w};
        CK(launch_hxv<VC>(T.s, T.path, T.col(T.Vb, cur), e, st));
      } else {
        EpiTrlLoc<VC> e{T.w, T.col(T.Vb, prv), pa + (k - 1), pb + (k - 1)};
        CK(launch_hxv<VC>(T.s, T.path, T.col(T.Vb, cur), e, st));
      }
      // alpha slot k, basis column cur; v_{k+1} = w / beta_k -> the window's other column
      CK(T.orth(k0 + 2, T.w, k, T.col(T.Vb, prv), k > 0 ? 1 : 0, cur));
    }
    const int n = k1 - k0s;
    HIPCK(hipMemcpyAsync(hal, pa + k0s, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(hbe, pb + k0s, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    al.insert(al.end(), hal, hal + n);
    be.insert(be.end(), hbe, hbe + n);
    const ScreenVerdict v = screen_decide(al, be, cut, tol);
    if (v == kScreenNone || v == kScreenBelow) *below = v;
    if (v != kScreenUndecided) return ED_OK;  // (QL failed: left undecided)
  }
  return ED_OK;
}

// sp_eigh replacement.  A single-vector Krylov method (ARPACK as much as this
// one) sees one direction of each degenerate eigenspace — the other copies
// only through rounding — so the lowest nev of a degenerate spectrum can come
// back with copies missing (configs[3] with the flat bath: 77 of 169
// sectors).  After the solve, the found vectors are locked and the lowest
// eigenvalue of H on their orthogonal complement is computed from a fresh
// random start (deflated solve); when it lies below the current nev-th value
// it is a missed eigenvalue and replaces it; repeated until a deflated solve
// finds nothing lower (ED_OPT_EIGH_NO_VERIFY skips this, A/B).
template <bool VC>
static int trlan_run(ed_sector* s, int nev, int ncv, int maxit, double tol, const void* v0,
                     double* evals, void* evecs, int32_t* nconv, int32_t* nhv) {
  using V = val_t<VC>;
  Trlan<VC> T;
  T.s = s;
  T.path = resolve_path(s, -1);
  T.st = s->stream;
  T.dim = s->dim;
  T.G = (int)std::min<int64_t>(grid_for(s->dim), s->dim > kTrlanBigDim ? 2 * kTrlanGridCap : kTrlanGridCap);
  T.fused = !(s->opts & ED_OPT_TRLAN_UNFUSED);
  if (s->opts & ED_OPT_TRLAN_NOFOLD) T.kFinFoldG = 0;
  T.graphs_on = !(s->opts & ED_OPT_NO_GRAPH);
  T.local = !(s->opts & ED_OPT_TRLAN_NOLOCAL);
  T.solo = !(s->opts & ED_OPT_TRLAN_NOSOLO);
  T.locupd = !(s->opts & ED_OPT_TRLAN_FULLUPD);
  const int64_t dim = s->dim;
  const int m = (int)std::min<int64_t>(ncv, dim);
  if (nev < 1 || nev >= m) return fail(ED_ERR_ARG, "need 1 <= nev < min(ncv, dim)");
  PinnedLease stage(TrlStage::kDoubles * sizeof(double), T.st);
  T.hp = (double*)stage.p;
  if (!T.hp) return fail(ED_ERR_OOM, "pinned host staging buffer");
  // the degeneracy probe's deflated solves need nev + mp basis columns
  const ScreenPlan may = screen_setup(m, nev, dim, s->opts, nev, 0.0, tol);
  const int mp = may.mp, mcap = may.verify ? std::max(m, nev + mp) : m;
  T.mcap = mcap;
  const size_t vs = sizeof(V);
  CK(T.alloc((void**)&T.Vb, (size_t)mcap * dim * vs));
  CK(T.alloc((void**)&T.w, dim * vs));
  CK(T.alloc((void**)&T.h, kTrlanMaxCols * sizeof(double2)));
  CK(T.alloc((void**)&T.coef, kTrlanMaxCols * sizeof(double2)));
  CK(T.alloc((void**)&T.part, (size_t)kTrlanMaxCols * T.G * sizeof(double2)));
  CK(T.alloc((void**)&T.part2, (size_t)kTrlanMaxCols * T.G * sizeof(double2)));
  CK(T.alloc((void**)&T.npart, (size_t)T.G * sizeof(double)));
  CK(T.alloc((void**)&T.npA, (size_t)T.G * sizeof(double)));
  CK(T.alloc((void**)&T.npB, (size_t)T.G * sizeof(double)));
  CK(T.alloc((void**)&T.lof, sizeof(int)));
  // alpha | beta in one block laid out as the staging: one copy down per restart
  CK(T.alloc((void**)&T.alpha, 2 * TrlStage::kBeta * sizeof(double)));
  T.beta = T.alpha + TrlStage::kBeta;
  CK(T.alloc((void**)&T.Y, (size_t)mcap * mcap * sizeof(double)));
  hipStream_t st = T.st;
  const int g = grid_for(dim);
  T.m = m;
  std::vector<double> theta, Z;
  int conv = 0;
  CK(trlan_core(T, 0, nev, maxit, tol, v0, 0, theta, Z, &conv));
  // Ritz vectors -> Vb[0, nev): the result vectors live there from here on
  // (locked columns of the deflated solves); with the probe also the next
  // Ritz vector -> Vb[nev] (the screen's start hint)
  double* const hZ = T.hp + TrlStage::kZ;
  std::copy(Z.begin(), Z.begin() + (size_t)m * m, hZ);
  HIPCK(hipMemcpyAsync(T.Y, hZ, (size_t)m * m * sizeof(double), hipMemcpyHostToDevice, st));
  const ScreenPlan sp = screen_setup(m, nev, dim, s->opts, conv, theta[nev - 1], tol);
  CK(T.rotate(0, m, sp.hint ? nev + 1 : nev, g));
  std::vector<double> ev(theta.begin(), theta.begin() + nev);
  if (sp.verify) {
    for (int round = 0; round < nev; round++) {
      // solve for the lowest eigenvalue on the complement of the nev vectors
      for (auto& gr : T.graphs) (void)hipGraphExecDestroy(gr.second);
      T.graphs.clear();  // captured sweeps depend on m
      T.m = nev + mp;
      std::vector<double> th2, Z2;
      int c2 = 0;
      const double cut = screen_cut(ev[nev - 1]);  // (a found copy moves ev[nev-1])
      if (!(s->opts & ED_OPT_EIGH_FULLPROBE)) {
        // cheap screen first: a plain Lanczos run on the complement decides
        // most sectors (no missed eigenvalue); the thick-restart probe below
        // runs only when it finds one or cannot decide
        int scr = -1;
        CK(probe_screen(T, nev, sp.maxsteps, sp.tprobe, cut, 3000 + round, &scr, sp.hint && round == 0));
        if (scr == 0) break;
      }
      // the thick-restart probe at the full tolerance: its converged Ritz
      // value lies within r^2/gap (r <= tol|theta|) of the complement's lowest
      // eigenvalue, so "th2 >= cut" is decided on an eigenvalue, not on a
      // loosely converged mixture of a near-cut cluster (round 5 ran it at
      // 1e-5 first and re-solved only below the cut)
      CK(trlan_core(T, nev, 1, maxit, tol, nullptr, 1000 + round, th2, Z2, &c2));
      if (!(c2 == 1 && th2[0] < cut)) break;
      const double mu = th2[0];
      // a missed eigenvalue: its Ritz vector -> w, then insert in order
      // (drop the current largest)
      const int ma2 = T.m - nev;
      std::copy(Z2.begin(), Z2.begin() + ma2, hZ);
      HIPCK(hipMemcpyAsync(T.Y, hZ, (size_t)ma2 * sizeof(double), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_rotate<VC>, dim3(std::min(g, 2048)), dim3(kBlock), (size_t)ma2 * sizeof(double), st,
                         T.col(T.Vb, nev), ma2, T.Y, ma2, 1, T.w, dim);
      HIPCK(hipGetLastError());
      int pos = nev - 1;
      while (pos > 0 && ev[pos - 1] > mu) pos--;
      for (int i = nev - 1; i > pos; i--) {
        ev[i] = ev[i - 1];
        HIPCK(hipMemcpyAsync(T.col(T.Vb, i), T.col(T.Vb, i - 1), dim * vs, hipMemcpyDeviceToDevice, st));
      }
      ev[pos] = mu;
      HIPCK(hipMemcpyAsync(T.col(T.Vb, pos), T.w, dim * vs, hipMemcpyDeviceToDevice, st));
    }
  }
  for (int i = 0; i < nev; i++) evals[i] = ev[i];
  // host or device destination (unified addressing): a farm keeps the
  // sector eigenvectors in HBM and copies back only the kept states
  if (evecs) HIPCK(hipMemcpyAsync(evecs, T.Vb, (size_t)nev * dim * vs, hipMemcpyDefault, st));
  HIPCK(hipStreamSynchronize(st));
  if (nconv) *nconv = conv;
  if (nhv) *nhv = T.nhv;
  return ED_OK;
}

// ------------------------------------------- batched small-sector eigh
// ed_sectors_eigh_batch: trlan_run's algorithm for many small stored sectors
// at once (ed_trlbatch.hpp): every restart cycle of every sector still in its
// main solve, and every 10-step chunk of every degeneracy screen, goes into
// one k_trl_batch launch; the host runs trlan_core's / probe_screen's
// decisions per sector on the mailbox values.  A sector the batch cannot
// finish (an invariant Krylov subspace, a screen that finds an eigenvalue
// below the cut or cannot decide, ED_OPT_EIGH_FULLPROBE) or cannot take
// (complex, not stored, beyond kTbMaxDim rows or kTbMaxCols columns) is
// solved afterwards by trlan_run on its own stream, from the same start.
struct TbSec {
  ed_sector* s = nullptr;
  int64_t dim = 0;
  int m = 0, it = 0, j0 = 0, conv = 0, nhv = 0;
  int state = 0;  // 0 main solve, 1 screen, 2 final rotation pending, 3 done, 4 fall back
  std::vector<double> Tm, theta, Z, ev, sal, sbe;
  ScreenPlan sp{};  // state 1
  TrlTask task{};
  int ny = 0;  // next launch's rotation: the first ny entries of Z (ld m)
};

static bool tb_eligible(const ed_sector* s, int nev, int ncv) {
  const int m = (int)std::min<int64_t>(ncv, s->dim);
  return s && !s->hc && s->nrows == s->dim && s->row0 == 0 && resolve_path(s, -1) == 0 && s->d_sptr &&
         s->d_diag && (s->d_words || (s->d_cols && s->d_vals)) && s->dim <= kTbMaxDim && m <= kTbMaxCols &&
         nev >= 1 && nev < m && nev + 2 <= kTbMaxCols && s->dim > (int64_t)nev + 2 && s->nslice * 64 >= s->dim &&
         // the multi-kernel A/B alternatives keep their own path
         !(s->opts & (ED_OPT_TRLAN_UNFUSED | ED_OPT_TRLAN_NOLOCAL | ED_OPT_TRLAN_NOSOLO));
}

// One sector's host step after a cycle of the batch (ed_trlbatch.hpp) or of
// the lockstep multi-sector solve (ed_trlmulti.hpp), on its mailbox ml
// (alpha [0, 32) | beta [32, 64) | scalar [64]): trlan_core's cycle with
// k0 = 0 and then probe_screen's, as a state machine over the same decisions
// (ed_hosteig.hpp); sets the sector's next task (b.task, b.ny).
static void tb_advance(TbSec& b, const double* ml, int nev, int maxit, double tol) {
  TrlTask& t = b.task;
  const int m = b.m;
  const double *al = ml, *be = ml + 32;
  b.ny = 0;
  if (b.state == 0) {  // a main sweep [j0, m) ran
    if (t.op == kTbStart && !(ml[64] > 0.0)) {
      b.state = 4;
      return;
    }
    b.nhv += m - b.j0;
    if (trl_fill(b.Tm.data(), m, 0, b.j0, m, al, be) >= 0) {
      b.state = 4;  // invariant subspace: trlan_run continues from a random direction
      return;
    }
    const double beta = be[m - 1];
    sym_eigh(m, b.Tm, b.theta, b.Z);
    b.conv = trl_nconv(m, nev, beta, b.theta.data(), b.Z.data(), tol);
    if (b.conv == nev || b.it == maxit - 1 || m == b.dim) {
      b.ev.assign(b.theta.begin(), b.theta.begin() + nev);
      const ScreenPlan sp = screen_setup(m, nev, b.dim, b.s->opts, b.conv, b.ev[nev - 1], tol);
      if (sp.verify && (b.s->opts & ED_OPT_EIGH_FULLPROBE)) {
        b.state = 4;
        return;
      }
      t.op = kTbScreen;
      t.ldy = m;
      t.nrot = sp.hint ? nev + 1 : nev;
      b.ny = m * t.nrot;
      t.k0s = 0;
      if (sp.verify) {
        b.state = 1;
        b.sp = sp;
        t.k1 = std::min(sp.maxsteps, kScreenChunk);
        t.hint = sp.hint ? 1 : 0;
        t.seed = 3000;
        b.sal.clear();
        b.sbe.clear();
      } else {
        b.state = 2;
        t.k1 = 0;
      }
      return;
    }
    const int nkeep = trl_nkeep(m, nev);
    t.op = kTbRestart;
    t.ldy = m;
    t.nrot = nkeep;
    b.ny = m * nkeep;
    trl_arrowhead(b.Tm.data(), m, nkeep, beta, b.theta.data(), b.Z.data());
    b.j0 = nkeep;
    b.it++;
    return;
  }
  if (b.state == 2) {  // the final rotation ran: done
    b.state = 3;
    return;
  }
  // a screen chunk [k0s, k1) ran
  const int nst = t.k1 - t.k0s;
  b.nhv += nst;
  b.sal.insert(b.sal.end(), al, al + nst);
  b.sbe.insert(b.sbe.end(), be, be + nst);
  t.nrot = 0;
  const ScreenVerdict v = screen_decide(b.sal, b.sbe, b.sp.cut, b.sp.tprobe);
  if (v == kScreenNone) b.state = 3;
  else if (v != kScreenUndecided || t.k1 >= b.sp.maxsteps) b.state = 4;
  else {
    t.k0s = t.k1;
    t.k1 = std::min(b.sp.maxsteps, t.k0s + kScreenChunk);
  }
}

// Fork-join helpers for the batch's per-sector host work (projected
// eigenproblem, screen QL): kept for one ed_sectors_eigh_batch call; the
// calling thread works too.  With dozens of sectors per cycle the host part
// was ~60 % of a batch (profiles/r6/batch_c4_timeline.json).
struct TbPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, cv_done;
  const std::function<void(int)>* fn = nullptr;
  std::atomic<int> next{0};
  int n = 0, gen = 0, busy = 0;
  bool quit = false;
  explicit TbPool(int nt) {
    for (int i = 0; i < nt; i++) th.emplace_back([this] { loop(); });
  }
  ~TbPool() {
    {
      std::lock_guard<std::mutex> g(mu);
      quit = true;
    }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
  void work() {
    for (int i; (i = next.fetch_add(1)) < n;) (*fn)(i);
  }
  void loop() {
    int seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return quit || gen != seen; });
      if (quit) return;
      seen = gen;
      lk.unlock();
      work();
      lk.lock();
      if (--busy == 0) cv_done.notify_one();
    }
  }
  void run(int count, const std::function<void(int)>& f) {
    if (th.empty() || count < 8) {
      for (int i = 0; i < count; i++) f(i);
      return;
    }
    {
      std::lock_guard<std::mutex> g(mu);
      fn = &f;
      n = count;
      next = 0;
      busy = (int)th.size();
      gen++;
    }
    cv.notify_all();
    work();
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return busy == 0; });
  }
};
static constexpr int kTbHostThreads = 3;  // helpers beside the calling thread

// Results of a batch / lockstep solve (S[k]: the call's sector idx[k], vectors
// in task.Vb); unfinished sectors go to `fallback`, re-solved by the caller.
static int tb_scatter(const std::vector<TbSec>& S, const std::vector<int>& idx, int nev, double* evals,
                      void* const* evecs, int32_t* nconv, int32_t* nhv, hipStream_t st, std::vector<int>& fallback) {
  for (size_t k = 0; k < S.size(); k++) {
    const TbSec& b = S[k];
    const int i = idx[k];
    if (nhv) nhv[i] = b.nhv;
    if (b.state != 3) {
      fallback.push_back(i);
      continue;
    }
    for (int e = 0; e < nev; e++) evals[(size_t)i * nev + e] = b.ev[e];
    if (evecs && evecs[i])
      HIPCK(hipMemcpyAsync(evecs[i], b.task.Vb, (size_t)nev * b.dim * sizeof(double), hipMemcpyDefault, st));
    if (nconv) nconv[i] = b.conv;
  }
  HIPCK(hipStreamSynchronize(st));
  return ED_OK;
}

static int tb_run(ed_sector* const* secs, const std::vector<int>& which, int nev, int ncv, const int32_t* maxits,
                  double tol, const double* const* v0, double* evals, void* const* evecs, int32_t* nconv,
                  int32_t* nhv, hipStream_t st, std::vector<int>& fallback) {
  std::vector<TbSec> S;
  std::vector<int> idx;
  for (int i : which) {
    if (!tb_eligible(secs[i], nev, ncv)) {
      fallback.push_back(i);
      continue;
    }
    TbSec b;
    b.s = secs[i];
    b.dim = secs[i]->dim;
    b.m = (int)std::min<int64_t>(ncv, b.dim);
    S.push_back(std::move(b));
    idx.push_back(i);
  }
  const int ns = (int)S.size();
  if (ns == 0) return ED_OK;
  // device: per sector Vb (mcap columns) | alpha, beta (72 each) | pa, pb
  // | coef | Y, each on a 16-byte boundary; the ws of all sectors contiguous
  // (one start-vector upload), the mailboxes too (one copy down per launch)
  size_t nw = 0, per = 0;
  std::vector<size_t> off(ns), woff(ns);
  for (int k = 0; k < ns; k++) {
    const int mcap = std::max(S[k].m, nev + 2);
    woff[k] = nw;
    nw += (size_t)S[k].dim;
    off[k] = per;
    per += even((size_t)mcap * S[k].dim) + 2 * TrlStage::kBeta + 2 * kTbScreenLen + 2 * kTrlanMaxCols +
           kTbMaxCols * kTbMaxCols;
  }
  const size_t nmail = (size_t)ns * kTbMail;
  const size_t ytot = (size_t)ns * kTbMaxCols * kTbMaxCols;  // rotations of one launch, packed
  const size_t bytes = (per + nw + nmail + ytot) * sizeof(double) + (size_t)ns * sizeof(TrlTask);
  char* dbase = nullptr;
  HIPCK(hipMallocAsync((void**)&dbase, bytes, st));
  DevFree free_guard{dbase, st};
  double* const dsec = (double*)dbase;
  double* const dw = dsec + per;
  double* const dmail = dw + nw;
  TrlTask* const dtask = (TrlTask*)(dmail + nmail);
  // pinned: start vectors | mailboxes | tasks + rotations of one launch
  // (the device mirrors the last part: [tasks | rotations packed])
  const size_t hbytes = (nw + nmail + ytot) * sizeof(double) + (size_t)ns * sizeof(TrlTask);
  PinnedLease stage(hbytes, st);
  char* const hp = (char*)stage.p;
  if (!hp) return fail(ED_ERR_OOM, "pinned staging (batch eigh)");
  double* const hv0 = (double*)hp;
  double* const hmail = hv0 + nw;
  TrlTask* const htask = (TrlTask*)(hmail + nmail);
  for (int k = 0; k < ns; k++) {
    TbSec& b = S[k];
    const ed_sector* s = b.s;
    double* p = dsec + off[k];
    const int mcap = std::max(b.m, nev + 2);
    TrlTask& t = b.task;
    t.diag = (const double*)s->d_diag;
    t.sptr = s->d_sptr;
    t.words = s->d_words;
    t.dict = (const double*)s->d_pdict;
    t.cols = s->d_cols;
    t.vals = (const double*)s->d_vals;
    t.dim = b.dim;
    t.Vb = p;
    p += even((size_t)mcap * b.dim);
    t.alpha = p;
    t.beta = p + TrlStage::kBeta;
    p += 2 * TrlStage::kBeta;
    t.pa = p;
    t.pb = p + kTbScreenLen;
    p += 2 * kTbScreenLen;
    t.coef = (double2*)p;
    p += 2 * kTrlanMaxCols;
    t.Y = p;
    t.w = dw + woff[k];
    t.mail = dmail + (size_t)k * kTbMail;
    t.m = b.m;
    t.nev = nev;
    t.locupd = !(s->opts & ED_OPT_TRLAN_FULLUPD);
    t.op = kTbStart;
    b.Tm.assign((size_t)b.m * b.m, 0.0);
    const int i = idx[k];
    if (v0 && v0[i]) memcpy(hv0 + woff[k], v0[i], b.dim * sizeof(double));
    else
      for (int64_t r = 0; r < b.dim; r++) hv0[woff[k] + r] = splitmix_unit((uint64_t)(r + 1));
  }
  HIPCK(hipMemcpyAsync(dw, hv0, nw * sizeof(double), hipMemcpyHostToDevice, st));
  static std::once_flag lds_once;
  static hipError_t lds_err = hipSuccess;
  std::call_once(lds_once, [] {
    lds_err = hipFuncSetAttribute((const void*)k_trl_batch<24>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kTbMaxDim * sizeof(double)));
    if (lds_err == hipSuccess)
      lds_err = hipFuncSetAttribute((const void*)k_trl_batch<32>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kTbMaxDim * sizeof(double)));
  });
  HIPCK(lds_err);
  std::vector<int> act;
  // per-sector host step after a launch (trlan_core's / probe_screen's logic)
  const std::function<void(int)> process = [&](int a) {
    const int k = act[a];
    tb_advance(S[k], hmail + (size_t)k * kTbMail, nev, maxits[idx[k]], tol);
  };
  TbPool pool(ns >= 8 ? kTbHostThreads : 0);
  for (;;) {
    act.clear();
    for (int k = 0; k < ns; k++)
      if (S[k].state <= 2) act.push_back(k);
    if (act.empty()) break;
    // tasks and rotations of this launch (rotations packed, one copy up)
    const int na = (int)act.size();
    double* const hY = (double*)(htask + na);
    const double* const dY = (const double*)(dtask + na);
    size_t yo = 0;
    int64_t maxdim = 0;
    int maxm = 0;
    for (int a = 0; a < na; a++) {
      TbSec& b = S[act[a]];
      TrlTask t = b.task;
      t.nrot = b.ny > 0 ? t.nrot : 0;
      if (b.ny > 0) {
        std::copy(b.Z.begin(), b.Z.begin() + b.ny, hY + yo);
        t.Y = dY + yo;
        yo += b.ny;
      }
      htask[a] = t;
      maxdim = std::max(maxdim, b.dim);
      maxm = std::max(maxm, std::max(b.m, nev + 2));
    }
    HIPCK(hipMemcpyAsync(dtask, htask, na * sizeof(TrlTask) + yo * sizeof(double), hipMemcpyHostToDevice, st));
    if (maxm <= 24)
      hipLaunchKernelGGL(k_trl_batch<24>, dim3((unsigned)na), dim3(kTbBlock), (size_t)maxdim * sizeof(double), st,
                         (const TrlTask*)dtask);
    else
      hipLaunchKernelGGL(k_trl_batch<32>, dim3((unsigned)na), dim3(kTbBlock), (size_t)maxdim * sizeof(double), st,
                         (const TrlTask*)dtask);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(hmail, dmail, nmail * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    pool.run((int)act.size(), process);
  }
  return tb_scatter(S, idx, nev, evals, evecs, nconv, nhv, st, fallback);
}

// ------------------------------------- lockstep multi-sector eigh
// tm_run: trlan_run's algorithm for stored sectors above the one-workgroup
// batch's size, all of them in lockstep (ed_trlmulti.hpp): one cycle = the
// rotations, then S steps of 7 launches each carrying every running sector,
// one mailbox copy down and the per-sector host step (tb_advance) on the
// pool.  Sectors it cannot take or finish go to `fallback`.
static bool tm_eligible(const ed_sector* s, int nev, int ncv) {
  const int m = (int)std::min<int64_t>(ncv, s->dim);
  return s && !s->hc && s->nrows == s->dim && s->row0 == 0 && resolve_path(s, -1) == 0 && s->d_sptr &&
         s->d_diag && s->d_words && s->d_pdict && m <= kTbMaxCols && nev >= 1 && nev < m &&
         nev + 2 <= kTbMaxCols && s->dim > (int64_t)nev + 2 && s->nslice * 64 >= s->dim &&
         !(s->opts & (ED_OPT_TRLAN_UNFUSED | ED_OPT_TRLAN_NOLOCAL | ED_OPT_TRLAN_NOSOLO));
}

static int tm_run(ed_sector* const* secs, const std::vector<int>& which, int nev, int ncv, const int32_t* maxits,
                  double tol, const double* const* v0, double* evals, void* const* evecs, int32_t* nconv,
                  int32_t* nhv, hipStream_t st, std::vector<int>& fallback) {
  const int ns = (int)which.size();
  if (ns == 0) return ED_OK;
  std::vector<TbSec> S(ns);
  std::vector<TmSec> hs(ns);
  std::vector<size_t> off(ns);
  size_t per = 0;
  for (int k = 0; k < ns; k++) {
    ed_sector* s = secs[which[k]];
    TbSec& b = S[k];
    b.s = s;
    b.dim = s->dim;
    b.m = (int)std::min<int64_t>(ncv, b.dim);
    b.Tm.assign((size_t)b.m * b.m, 0.0);
    // (as one sector's sweep alone, at most kTrlanGridCap blocks: every block
    // of the DGKS and local-only decisions sums all G partials; ~2,048 rows
    // per block below that)
    const int G = (int)std::max<int64_t>(
        1, std::min<int64_t>((b.dim + kTmRowsPerBlock - 1) / kTmRowsPerBlock, kTrlanGridCap));
    hs[k].G = G;
    hs[k].Gh = (int)std::min<int64_t>((b.dim + 4 * kBlock - 1) / (4 * kBlock), 4096);  // 4 rows per thread
    const int mcap = std::max(b.m, nev + 2);
    off[k] = per;
    // (every sub-array starts on a 16-byte boundary: the double2 ones need it)
    per += even((size_t)mcap * b.dim) + even(b.dim) + 4 * (size_t)kTrlanMaxCols * G + even(3 * (size_t)G) +
           4 * kTrlanMaxCols + 2 + 2 * TrlStage::kBeta + 2 * kTbScreenLen;
  }
  const size_t nmail = (size_t)ns * kTbMail;
  const size_t ytot = (size_t)ns * kTbMaxCols * kTbMaxCols;
  const size_t ctab = (size_t)ns * sizeof(TmCyc) + 2 * (ns + 1) * sizeof(int) + 64;
  const size_t bytes = (per + nmail + ytot) * sizeof(double) + (size_t)ns * sizeof(TmSec) + ctab;
  char* dbase = nullptr;
  HIPCK(hipMallocAsync((void**)&dbase, bytes, st));
  DevFree free_guard{dbase, st};
  double* const dsec = (double*)dbase;
  double* const dmail = dsec + per;
  TmSec* const dtab = (TmSec*)(dmail + nmail);
  char* const dcyc = (char*)(dtab + ns);  // [TmCyc | boffG | boffH | pad | Y packed] of one cycle
  // pinned: start column / mailboxes | cycle table
  const int64_t maxdim = [&] { int64_t d = 0; for (auto& b : S) d = std::max(d, b.dim); return d; }();
  const size_t hbytes = std::max<size_t>(maxdim, nmail) * sizeof(double) + ctab + ytot * sizeof(double);
  PinnedLease stage(hbytes, st);
  char* const hp = (char*)stage.p;
  if (!hp) return fail(ED_ERR_OOM, "pinned staging (multi-sector eigh)");
  double* const hmail = (double*)hp;
  char* const hcyc = hp + std::max<size_t>(maxdim, nmail) * sizeof(double);
  for (int k = 0; k < ns; k++) {
    TbSec& b = S[k];
    const ed_sector* s = b.s;
    TmSec& t = hs[k];
    double* p = dsec + off[k];
    const int mcap = std::max(b.m, nev + 2);
    t.diag = (const double*)s->d_diag;
    t.sptr = s->d_sptr;
    t.words = s->d_words;
    t.dict = (const double*)s->d_pdict;
    t.dim = b.dim;
    // (columns at stride dim, as the sweeps index them; each sub-array starts
    // on a 16-byte boundary)
    t.Vb = p;
    b.task.Vb = p;  // (tb_scatter)
    p += even((size_t)mcap * b.dim);
    t.w = p;
    p += even(b.dim);
    t.part = (double2*)p;
    p += 2 * (size_t)kTrlanMaxCols * t.G;
    t.part2 = (double2*)p;
    p += 2 * (size_t)kTrlanMaxCols * t.G;
    t.npA = p;
    t.npB = p + t.G;
    t.npart = p + 2 * t.G;
    p += even(3 * (size_t)t.G);
    t.h = (double2*)p;
    t.coef = (double2*)(p + 2 * kTrlanMaxCols);
    p += 4 * kTrlanMaxCols;
    t.lof = (int*)p;
    p += 2;
    t.alpha = p;
    t.beta = p + TrlStage::kBeta;
    t.pa = p + 2 * TrlStage::kBeta;
    t.pb = t.pa + kTbScreenLen;
    t.mail = dmail + (size_t)k * kTbMail;
    b.task.m = b.m;
    b.task.nev = nev;
    b.task.locupd = !(s->opts & ED_OPT_TRLAN_FULLUPD);
    b.task.op = kTbStart;
    // V_0 = v0 / |v0| (host norm)
    double* h0 = (double*)hp;
    const int i = which[k];
    double n2 = 0.0;
    for (int64_t r = 0; r < b.dim; r++) {
      h0[r] = (v0 && v0[i]) ? v0[i][r] : splitmix_unit((uint64_t)(r + 1));
      n2 += h0[r] * h0[r];
    }
    if (!(n2 > 0.0)) {
      b.state = 4;
      continue;
    }
    const double inv = 1.0 / sqrt(n2);
    for (int64_t r = 0; r < b.dim; r++) h0[r] *= inv;
    HIPCK(hipMemcpyAsync(t.Vb, h0, b.dim * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));  // (the staging buffer is reused for the next sector)
  }
  HIPCK(hipMemcpyAsync(dtab, hs.data(), ns * sizeof(TmSec), hipMemcpyHostToDevice, st));
  std::vector<int> act;
  const std::function<void(int)> process = [&](int a) {
    const int k = act[a];
    tb_advance(S[k], hmail + (size_t)k * kTbMail, nev, maxits[which[k]], tol);
  };
  TbPool pool(ns >= 8 ? kTbHostThreads : 0);
  for (;;) {
    act.clear();
    for (int k = 0; k < ns; k++)
      if (S[k].state <= 2) act.push_back(k);
    if (act.empty()) break;
    const int na = (int)act.size();
    TmCyc* const hc = (TmCyc*)hcyc;
    int* const hboG = (int*)(hc + na);
    int* const hboH = hboG + (na + 1);
    const size_t yoff = ((na * sizeof(TmCyc) + 2 * (na + 1) * sizeof(int)) + 63) / 64 * 64;
    double* const hY = (double*)(hcyc + yoff);
    const double* const dY = (const double*)(dcyc + yoff);
    size_t yo = 0;
    int steps = 0, maxm = 0, bG = 0, bH = 0;
    bool rot = false;
    for (int a = 0; a < na; a++) {
      TbSec& b = S[act[a]];
      const TrlTask& t = b.task;
      TmCyc c{};
      c.sec = act[a];
      c.m = b.m;
      c.nev = nev;
      c.locupd = t.locupd;
      c.scale_col = -1;
      c.ldy = t.ldy;
      c.nrot = b.ny > 0 ? t.nrot : 0;
      if (t.op == kTbStart) {
        c.phase = 0;
        c.j0 = 0;
      } else if (t.op == kTbRestart) {
        c.phase = 0;
        c.j0 = t.nrot;
        c.scale_col = t.nrot;
      } else {
        c.phase = 1;
        c.k0s = t.k0s;
        c.k1 = t.k1;
        c.sstart = (t.k0s == 0 && t.k1 > 0) ? 1 : 0;
        c.hint = t.hint;
        c.seed = t.seed;
      }
      if (b.ny > 0) {
        std::copy(b.Z.begin(), b.Z.begin() + b.ny, hY + yo);
        c.Y = dY + yo;
        yo += b.ny;
      }
      rot = rot || c.nrot > 0 || c.scale_col >= 0;
      steps = std::max(steps, c.phase == 0 ? c.m - c.j0 : c.k1 - c.k0s + c.sstart);
      maxm = std::max(maxm, c.phase == 0 ? c.m : nev + 2);
      hc[a] = c;
      hboG[a] = bG;
      hboH[a] = bH;
      bG += hs[act[a]].G;
      bH += hs[act[a]].Gh;
    }
    hboG[na] = bG;
    hboH[na] = bH;
    HIPCK(hipMemcpyAsync(dcyc, hcyc, yoff + yo * sizeof(double), hipMemcpyHostToDevice, st));
    const TmCyc* dc = (const TmCyc*)dcyc;
    const int* dboG = (const int*)(dc + na);
    const int* dboH = dboG + (na + 1);
    if (rot) hipLaunchKernelGGL(k_tm_rotate, dim3(bG), dim3(kBlock), 0, st, dtab, dc, dboG, na);
    for (int q = 0; q < steps; q++) {
      hipLaunchKernelGGL(k_tm_hxv, dim3(bH), dim3(kBlock), 0, st, dtab, dc, dboH, na, q);
      for (int pass = 1; pass <= 3; pass++) {
        if (maxm <= 24) hipLaunchKernelGGL(k_tm_cgs<24>, dim3(bG), dim3(kBlock), 0, st, dtab, dc, dboG, na, q, pass);
        else hipLaunchKernelGGL(k_tm_cgs<32>, dim3(bG), dim3(kBlock), 0, st, dtab, dc, dboG, na, q, pass);
        if (pass < 3)
          hipLaunchKernelGGL(k_tm_fin, dim3(na * kTmFinBlocks), dim3(kBlock), 0, st, dtab, dc, na, q, pass);
      }
      hipLaunchKernelGGL(k_tm_coef, dim3(bG), dim3(kBlock), 0, st, dtab, dc, dboG, na, q);
    }
    hipLaunchKernelGGL(k_tm_mail, dim3(na), dim3(64), 0, st, dtab, dc);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(hmail, dmail, nmail * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    pool.run(na, process);
  }
  return tb_scatter(S, which, nev, evals, evecs, nconv, nhv, st, fallback);
}

extern "C" {

int ed_sectors_eigh_batch(ed_sector* const* secs, int32_t n, int32_t nev, int32_t ncv, const int32_t* maxit,
                          double tol, const double* const* v0, double* evals, void* const* evecs, int32_t* nconv,
                          int32_t* nhv, int32_t* nbatched, int32_t flags, void* stream) {
  if (!secs || n < 0 || !evals || !maxit) return fail(ED_ERR_ARG, "bad args");
  for (int i = 0; i < n; i++)
    if (maxit[i] < 1) return fail(ED_ERR_ARG, "maxit < 1");
  if (n == 0) return ED_OK;
  if (ncv > kTrlanMaxCols) return fail(ED_ERR_ARG, "ncv > 64 not supported");
  for (int i = 0; i < n; i++) {
    if (!secs[i]) return fail(ED_ERR_ARG, "null sector");
    CK(whole_only(secs[i]));
    if (secs[i]->hc) return fail(ED_ERR_ARG, "batched eigh: real vectors only (complex H needs vtype=1)");
    if (secs[i]->device != secs[0]->device) return fail(ED_ERR_ARG, "batched eigh: sectors on different devices");
  }
  const int dev = secs[0]->device;
  HIPCK(hipSetDevice(dev));
  hipStream_t st = stream ? (hipStream_t)stream : secs[0]->stream;
  // up to kTbWgMaxDim rows: one workgroup per sector (ed_trlbatch.hpp), on a
  // second stream from a helper thread; larger: the lockstep multi-sector
  // solve (ed_trlmulti.hpp) here; the rest one by one afterwards
  std::vector<int> small, multi, fb, fb_small;
  for (int i = 0; i < n; i++) {
    if (secs[i]->dim <= kTbWgMaxDim && tb_eligible(secs[i], nev, ncv)) small.push_back(i);
    else if (tm_eligible(secs[i], nev, ncv)) multi.push_back(i);
    else fb.push_back(i);
  }
  int rc_small = ED_OK;
  std::string err_small;
  std::thread th;
  hipStream_t st2 = nullptr;
  if (!small.empty()) {
    if (multi.empty()) {
      rc_small = tb_run(secs, small, nev, ncv, maxit, tol, v0, evals, evecs, nconv, nhv, st, fb_small);
    } else {
      HIPCK(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
      th = std::thread([&] {
        if (hipSetDevice(dev) != hipSuccess) rc_small = ED_ERR_HIP;
        else rc_small = tb_run(secs, small, nev, ncv, maxit, tol, v0, evals, evecs, nconv, nhv, st2, fb_small);
        if (rc_small != ED_OK) err_small = ed_err_slot();
      });
    }
  }
  int rc_multi = ED_OK;
  for (size_t c0 = 0; c0 < multi.size() && rc_multi == ED_OK; c0 += kTmMaxEntries) {
    const std::vector<int> part(multi.begin() + c0, multi.begin() + std::min(multi.size(), c0 + kTmMaxEntries));
    rc_multi = tm_run(secs, part, nev, ncv, maxit, tol, v0, evals, evecs, nconv, nhv, st, fb);
  }
  if (th.joinable()) th.join();
  if (st2) (void)hipStreamDestroy(st2);
  if (rc_multi != ED_OK) return rc_multi;
  if (rc_small != ED_OK) return fail(rc_small, err_small.empty() ? ed_err_slot() : err_small);
  fb.insert(fb.end(), fb_small.begin(), fb_small.end());
  if (nbatched) *nbatched = n - (int)fb.size();
  if (flags & ED_BATCH_NO_FALLBACK) {  // the caller solves them (nconv -1)
    for (int i : fb)
      if (nconv) nconv[i] = -1;
    return ED_OK;
  }
  for (int i : fb) {
    int32_t c = 0, h = 0;
    CK(trlan_run<false>(secs[i], nev, ncv, maxit[i], tol, v0 ? v0[i] : nullptr, evals + (size_t)i * nev,
                        evecs ? evecs[i] : nullptr, &c, &h));
    if (nconv) nconv[i] = c;
    if (nhv) nhv[i] += h;
  }
  return ED_OK;
}

int ed_sector_eigh(ed_sector* s, int32_t vtype, int32_t nev, int32_t ncv, int32_t maxit,
                              double tol, const void* v0, double* evals, void* evecs, int32_t* nconv,
                              int32_t* nhv) {
  if (!s || !evals || maxit < 1) return fail(ED_ERR_ARG, "bad args");
  CK(whole_only(s));
  if (vtype == 0 && s->hc) return fail(ED_ERR_ARG, "complex H needs vtype=1");
  if (ncv > kTrlanMaxCols) return fail(ED_ERR_ARG, "ncv > 64 not supported");
  HIPCK(hipSetDevice(s->device));
  return with_vc(vtype, [&](auto c) {
    return trlan_run<decltype(c)::value>(s, nev, ncv, maxit, tol, v0, evals, evecs, nconv, nhv);
  });
}

}  // extern "C"
