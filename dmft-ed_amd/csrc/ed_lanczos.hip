// ed_lanczos.hip — the Lanczos workspace of a sector (ed_sector.hpp), the
// plain multi-kernel recurrence (graph-captured in chunks), the persistent
// one-workgroup recurrence of small sectors (kernel: ed_persist.hpp, launch:
// ed_persist_launch.hip), the driver that chooses between them, and the
// Lanczos entry points of the C-ABI (include/ed_gpu.h).
#include "ed_sector.hpp"
#include "ed_persist.hpp"
#include "ed_hosteig.hpp"
#include "ed_multi.hpp"
#include "ed_lockstep_groups.hpp"

using namespace edg;

// ------------------------------------------------------------ Lanczos
void drop_graph(ed_sector* s) {
  // a captured graph bakes in buffer pointers: any workspace reallocation
  // invalidates it
  if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
  s->gexec = nullptr;
}

// P (= v_{k-1}) is read by every row slot of the register-mode persistent
// kernels, padding rows included (a guarded load per row costs spills): it
// has at least kPRegBlock * 10 rows, the padding kept zero by the kernel.
static size_t p_rows(const ed_sector* s) { return (size_t)std::max<int64_t>(s->dim, (int64_t)kPRegBlock * 10); }

static int lanc_prepare(ed_sector* s, int vc, int cap, bool want_basis, int basis_cols) {
  LancWS& w = s->ws;
  const size_t vs = vc ? 16 : 8;
  if (w.vc != vc) {
    drop_graph(s);
    if (w.vc != -1) {  // switching real <-> complex vectors: re-size the vector buffers
      HIPCK(hipStreamSynchronize(s->stream));
      const size_t ovs = w.vc ? 16 : 8;
      dfree(s, &w.R, s->dim * ovs);
      dfree(s, &w.P, p_rows(s) * ovs);
      dfree(s, &w.W, s->dim * ovs);
      dfree(s, &w.Y, s->dim * ovs);
      dfree(s, &w.basis, (size_t)w.basis_cols * s->dim * ovs);
      w.basis_cols = 0;
      CK(dalloc(s, &w.R, s->dim * vs));
      CK(dalloc(s, &w.P, p_rows(s) * vs));
      CK(dalloc(s, &w.W, s->dim * vs));
      CK(dalloc(s, &w.Y, s->dim * vs));
      w.vc = vc;
      goto sized;
    }
    CK(dalloc(s, &w.R, s->dim * vs));
    CK(dalloc(s, &w.P, p_rows(s) * vs));
    CK(dalloc(s, &w.W, s->dim * vs));
    CK(dalloc(s, &w.Y, s->dim * vs));
    CK(dalloc_t(s, &w.st, 1));
    CK(dalloc_t(s, &w.partials, kMaxGrid));
    CK(dalloc_t(s, &w.counter, 4));
    HIPCK(hipMemsetAsync(w.counter, 0, 4 * sizeof(unsigned int), s->stream));  // stream-ordered: s->stream does not sync with the null stream
    w.vc = vc;
  }
sized:
  if (cap > w.cap) {
    drop_graph(s);
    double* blk = nullptr;
    CK(dalloc_t(s, &blk, 3 * ((size_t)cap + 2)));
    w.alpha = blk;
    w.beta = blk + (cap + 2);
    w.z = blk + 2 * ((size_t)cap + 2);
    if (w.h_ab) {
      HIPCK(hipStreamSynchronize(s->stream));  // no copy into the old staging in flight
      pinned_put(w.h_ab);
      w.h_ab = nullptr;
    }
    w.h_ab = (double*)pinned_get(2 * ((size_t)cap + 2) * sizeof(double));
    if (!w.h_ab) return fail(ED_ERR_OOM, "pinned host staging");
    w.cap = cap;
  }
  if (want_basis && basis_cols > w.basis_cols) {
    drop_graph(s);
    CK(dalloc(s, &w.basis, (size_t)basis_cols * s->dim * vs));
    w.basis_cols = basis_cols;
  }
  return ED_OK;
}

// splitmix64 hash start vector in [-1,1) (documented in DESIGN.md; tests reproduce it)
__global__ void k_default_start(double* v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    v[i] = splitmix_unit((uint64_t)(i + 1));
  }
}

void launch_default_start(double* v, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_default_start, dim3(grid_for(n)), dim3(kBlock), 0, st, v, n);
}

namespace edg {
// Two-pass finishing kernels of one Lanczos step (one block of kBlock threads).
static __global__ void __launch_bounds__(kBlock) k_lanc_fin_a(const double* __restrict__ partials, int n,
                                                       LancState* st, double* alpha_out) {
  if (st->done) return;
  const double tot = sum_partials(partials, n);
  if (threadIdx.x == 0) {
    st->alpha = tot;
    alpha_out[st->iter] = tot;
  }
}
static __global__ void __launch_bounds__(kBlock) k_lanc_fin_b(const double* __restrict__ partials, int n,
                                                       LancState* st, double* beta_out) {
  if (st->done) return;
  const double tot = sum_partials(partials, n);
  if (threadIdx.x == 0) lanc_set_beta(tot, st, beta_out);
}
}  // namespace edg

template <bool VC>
static int lanc_start(ed_sector* s, double thresh, hipStream_t st) {
  LancWS& w = s->ws;
  RedSlot slot{w.partials, w.counter};
  HIPCK(hipMemsetAsync(w.alpha, 0, 2 * (w.cap + 2) * sizeof(double), st));  // alpha | beta
  hipLaunchKernelGGL(k_lanc_init<VC>, dim3(grid_once(s->dim)), dim3(kBlock), 0, st,
                     (const val_t<VC>*)w.R, (val_t<VC>*)w.P, s->dim, w.st, thresh, slot);
  HIPCK(hipGetLastError());
  return ED_OK;
}

template <bool VC>
static int lanc_iter(ed_sector* s, int path, bool basis, hipStream_t st) {
  LancWS& w = s->ws;
  const int g1 = hxv_blocks(s, path, VC), g2 = grid_for(s->dim);
  const bool two1 = g1 > kTicketMaxBlocks, two2 = g2 > kTicketMaxBlocks;
  EpiLancA<VC> e;
  e.st = w.st;
  e.P = (val_t<VC>*)w.P;
  e.W = (val_t<VC>*)w.W;
  e.basis = basis ? (val_t<VC>*)w.basis : nullptr;
  e.dim = s->dim;
  e.alpha_out = w.alpha;
  e.slot = RedSlot{w.partials, two1 ? nullptr : w.counter};
  CK(launch_hxv<VC>(s, path, w.R, e, st));
  if (two1) hipLaunchKernelGGL(k_lanc_fin_a, dim3(1), dim3(kBlock), 0, st, w.partials, g1, w.st, w.alpha);
  RedSlot slot2{w.partials, two2 ? nullptr : w.counter + 1};
  hipLaunchKernelGGL(k_lanc_b<VC>, dim3(g2), dim3(kBlock), 0, st, (const val_t<VC>*)w.W,
                     (const val_t<VC>*)w.P, (val_t<VC>*)w.R, s->dim, w.st, w.beta, slot2);
  if (two2) hipLaunchKernelGGL(k_lanc_fin_b, dim3(1), dim3(kBlock), 0, st, w.partials, g2, w.st, w.beta);
  HIPCK(hipGetLastError());
  return ED_OK;
}

// Run n iterations on stream st; graph-captured in chunks when st is the
// sector's private stream (launch-bound small sectors).
template <bool VC>
static int lanc_iters(ed_sector* s, int path, bool basis, int n, hipStream_t st) {
  const int chunk = 32;
  if (st != s->stream || n < chunk) {
    for (int k = 0; k < n; k++) CK((lanc_iter<VC>(s, path, basis, st)));
    return ED_OK;
  }
  if (!s->gexec || s->g_path != path || s->g_vc != (int)VC || s->g_basis != basis ||
      s->g_chunk != chunk) {
    if (s->gexec) {
      (void)hipGraphExecDestroy(s->gexec);
      s->gexec = nullptr;
    }
    hipGraph_t g;
    HIPCK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = ED_OK;
    for (int k = 0; k < chunk && rc == ED_OK; k++) rc = lanc_iter<VC>(s, path, basis, st);
    hipError_t e2 = hipStreamEndCapture(st, &g);
    if (rc != ED_OK) return rc;
    HIPCK(e2);
    HIPCK(hipGraphInstantiate(&s->gexec, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    s->g_path = path;
    s->g_vc = VC;
    s->g_basis = basis;
    s->g_chunk = chunk;
  }
  int k = 0;
  for (; k + chunk <= n; k += chunk) HIPCK(hipGraphLaunch(s->gexec, st));
  for (; k < n; k++) CK((lanc_iter<VC>(s, path, basis, st)));
  return ED_OK;
}

// ---------------------------------------------- persistent small-sector path
static constexpr int64_t kLdsBudget = 150 * 1024;

// MODE 2 packing (ELL in registers): row i = t + r*kPRegBlock of thread t
// keeps W words {col:17 | dictionary byte offset:14}, W = the smallest of
// 8/12/14/16 >= the longest row, padded with entry (col 0, dict[0] = 0.0).
// The dictionary holds the distinct values by bit pattern: exact.
static int build_preg(ed_sector* s) {
  if (s->preg_E) return s->preg_E;
  s->preg_E = -1;
  const int64_t dim = s->dim, ns = s->nslice, slots = s->padded;
  if (!(s->flags & ED_STORED) || dim > 10 * (int64_t)kPRegBlock) return -1;
  const int hw = s->hc ? 2 : 1;
  std::vector<uint16_t> cnt(dim);
  std::vector<int64_t> sptr(ns + 1);
  std::vector<int32_t> sc(slots);
  std::vector<double> sv(slots * hw);
  HIPCK(hipStreamSynchronize(s->stream));  // SELL arrays come from kernels on s->stream
  CK(dcopy(s, cnt.data(), s->d_cnt, dim * 2, hipMemcpyDeviceToHost));
  CK(dcopy(s, sptr.data(), s->d_sptr, (ns + 1) * 8, hipMemcpyDeviceToHost));
  CK(dcopy(s, sc.data(), s->d_cols, slots * 4, hipMemcpyDeviceToHost));
  CK(dcopy(s, sv.data(), s->d_vals, slots * 8 * hw, hipMemcpyDeviceToHost));
  if (hw == 2) {  // the register modes keep a real diagonal (Hermitian H)
    std::vector<double> dg(dim * 2);
    CK(dcopy(s, dg.data(), s->d_diag, dim * 16, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < dim; i++)
      if (dg[2 * i + 1] != 0.0) return -1;
  }
  int wmax = 0;
  for (int64_t i = 0; i < dim; i++) wmax = std::max<int>(wmax, cnt[i]);
  int W = 0;
  for (int w : {8, 12, 14, 16})
    if (!W && wmax <= w) W = w;
  if (!W) return -1;
  const int64_t rpt = (dim + kPRegBlock - 1) / kPRegBlock;
  const int RPT = rpt <= 2 ? 2 : rpt <= 4 ? 4 : rpt <= 6 ? 6 : rpt <= 8 ? 8 : 10;
  const uint32_t hs = s->hc ? 16 : 8;
  std::map<std::pair<uint64_t, uint64_t>, uint32_t> idx;
  std::vector<double> dict(hw, 0.0);
  idx[{0, 0}] = 0;
  std::vector<uint32_t> pk((size_t)RPT * W * kPRegBlock, 0u);
  for (int64_t i = 0; i < dim; i++) {
    const int t = (int)(i % kPRegBlock), r = (int)(i / kPRegBlock);
    const int64_t base = sptr[i >> 6] + (i & 63);
    for (int k = 0; k < cnt[i]; k++) {
      const int64_t q = base + 64 * (int64_t)k;
      uint64_t x0 = 0, x1 = 0;
      memcpy(&x0, &sv[hw * q], 8);
      if (hw == 2) memcpy(&x1, &sv[2 * q + 1], 8);
      auto it = idx.find({x0, x1});
      uint32_t id;
      if (it == idx.end()) {
        id = (uint32_t)idx.size();
        if ((id + 1) * hs > kPkOffMask + 1) return -1;
        idx[{x0, x1}] = id;
        for (int c = 0; c < hw; c++) dict.push_back(sv[hw * q + c]);
      } else {
        id = it->second;
      }
      pk[((size_t)r * W + k) * kPRegBlock + t] = (uint32_t)sc[q] | ((id * hs) << kPkColBits);
    }
  }
  CK(dalloc(s, (void**)&s->d_pk, pk.size() * 4));
  CK(dalloc(s, &s->d_dict, dict.size() * 8));
  CK(dcopy(s, s->d_pk, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
  CK(dcopy(s, s->d_dict, dict.data(), dict.size() * 8, hipMemcpyHostToDevice));
  s->ndict = (int)(dict.size() / hw);
  s->preg_E = W;
  s->preg_rpt = RPT;
  return W;
}

// MODE 4 (Kronecker register layout, ed_persist.hpp): per lane E up-hop
// entries once plus RPT rows x (E down-hop entries, diagonal, r, p, w) must
// stay below the spill-free budget (-Rpass-analysis=kernel-resource-usage:
// E=4/RPT=10 and E=8/RPT=6 compile without scratch).
// complex vectors (1024 threads, <= 128 VGPRs): per row the down-hop byte
// offsets and the complex w and p; the diagonal and the hop values in LDS
// (-Rpass-analysis: E=4 up to 5 rows, E=8 up to 3 rows spill-free)
static int pkr_geom(ed_sector* s, int64_t du, int64_t dd, int degu, int degd) {
  const int deg = std::max(degu, degd);
  const int E = deg <= 4 ? 4 : deg <= 8 ? 8 : 0;
  if (!E || du < 1 || du > kPRegBlock || du * dd != s->dim) return -1;
  const int64_t G = kPRegBlock / du, rpt = (dd + G - 1) / G;
  const int RPT = rpt <= 2 ? 2 : rpt <= 4 ? 4 : rpt <= 6 ? 6 : rpt <= 8 ? 8 : rpt <= 10 ? 10 : 0;
  if (!RPT || !pkr_fits(E, RPT)) return -1;
  s->pkr_E = E;
  s->pkr_rpt = RPT;
  s->pkr_du = (int)du;
  s->pkr_dd = (int)dd;
  s->pkr_degu = degu;
  s->pkr_degd = degd;
  return 1;
}

// MODE 4 up-hop slot order.  Slot e of every lane is gathered by one
// ds_read_b64 per row; its 32-lane halves hit bank pair (g*DimUp + target)
// mod 32 (the iw*DimUp part common to a wave's rows drops out, so one order
// serves every row slot r), and each extra distinct address on a bank pair
// costs one LDS cycle.  The up list of iu is shared by the G lanes (g, iu):
// permute each list (all orders for E=4, pairwise swaps for E=8) to minimise
// the summed conflict cycles over the halves containing one of its lanes.
// Entries stay the same (target, value) pairs, so H is unchanged; only the
// per-row summation order moves.  configs[1]: 1150 -> ~890 LDS cycles/step.
using PkrHop = std::pair<int32_t, uint64_t>;
static void pkr_order_up(std::vector<std::vector<PkrHop>>& ul, int du, int E) {
  const int G = kPRegBlock / du;
  for (auto& l : ul) l.resize(E, PkrHop{0, 0});  // padding: (col 0, 0.0) reads the row base
  auto half_cost = [&](int h, int e) {
    int nb[32] = {0}, cyc = 0;
    int seen[32][32];
    for (int l = 0; l < 32; l++) {
      const int t = 32 * h + l;
      if (t >= G * du) break;
      const int g = t / du, iu = t - g * du;
      const int addr = g * du + ul[iu][e].first, b = addr & 31;
      bool dup = false;
      for (int k = 0; k < nb[b]; k++) dup |= seen[b][k] == addr;
      if (!dup) { seen[b][nb[b]++] = addr; cyc = std::max(cyc, nb[b]); }
    }
    return cyc;
  };
  auto cost_of = [&](int iu) {
    int c = 0;
    for (int g = 0; g < G; g++) {
      const int h = (g * du + iu) / 32;
      for (int e = 0; e < E; e++) c += half_cost(h, e);
    }
    return c;
  };
  for (int sweep = 0; sweep < 3; sweep++) {
    bool moved = false;
    for (int iu = 0; iu < du; iu++) {
      std::vector<PkrHop>& l = ul[iu];
      int best = cost_of(iu);
      if (E <= 4) {
        std::vector<PkrHop> cur = l, keep = l;
        std::sort(cur.begin(), cur.end());
        do {
          l = cur;
          const int c = cost_of(iu);
          if (c < best) { best = c; keep = cur; moved = true; }
        } while (std::next_permutation(cur.begin(), cur.end()));
        l = keep;
      } else {
        for (int a = 0; a < E; a++)
          for (int b = a + 1; b < E; b++) {
            std::swap(l[a], l[b]);
            const int c = cost_of(iu);
            if (c < best) { best = c; moved = true; } else { std::swap(l[a], l[b]); }
          }
      }
    }
    if (!moved) break;
  }
}

static int pkr_upload(ed_sector* s, const std::vector<std::vector<PkrHop>>& L, int deg, int64_t n,
                      const int32_t** dc, const double** dv) {
  std::vector<int32_t> c((size_t)std::max(deg, 1) * n, 0);
  std::vector<double> v((size_t)std::max(deg, 1) * n, 0.0);
  for (int64_t r = 0; r < n; r++)
    for (size_t e = 0; e < L[r].size() && (int)e < deg; e++) {
      c[e * n + r] = L[r][e].first;
      memcpy(&v[e * n + r], &L[r][e].second, 8);
    }
  int32_t* pc;
  void* pv;
  CK(upload(s, &pc, c));
  CK(dalloc(s, &pv, v.size() * 8));
  CK(dcopy(s, pv, v.data(), v.size() * 8, hipMemcpyHostToDevice));
  *dc = pc;
  *dv = (const double*)pv;
  return ED_OK;
}

// MODE 4 tables of a stored sector: read back from the stored SELL matrix
// and accepted only when it has the Kronecker form H = D + Hup(x)1 + 1(x)Hdw
// on the DimDw x DimUp view (row = iw*DimUp + iu): every entry of row
// (iw, iu) keeps iw (up hop) or iu (down hop), the up list of iu is the same
// (targets and value bits, in order) in every iw block and the down list of
// iw the same for every iu.  The registers then hold exactly the stored
// values; only the summation order (diag, up, down) differs from k_spmv.
static int build_pkron_stored(ed_sector* s) {
  if (s->pkr_state && s->pkr_src == 0) return s->pkr_state;
  s->pkr_state = -1;
  s->pkr_src = 0;
  if (s->hc || s->Mh.mode != ED_MODE_NORMAL || !(s->flags & ED_STORED)) return -1;
  const int64_t du = s->T.dimup, dd = s->T.dimdw, dim = s->dim, ns = s->nslice, slots = s->padded;
  if (du < 1 || du > kPRegBlock || du * dd != dim) return -1;
  std::vector<uint16_t> cnt(dim);
  std::vector<int64_t> sptr(ns + 1);
  std::vector<int32_t> sc(slots);
  std::vector<double> sv(slots);
  HIPCK(hipStreamSynchronize(s->stream));
  CK(dcopy(s, cnt.data(), s->d_cnt, dim * 2, hipMemcpyDeviceToHost));
  CK(dcopy(s, sptr.data(), s->d_sptr, (ns + 1) * 8, hipMemcpyDeviceToHost));
  CK(dcopy(s, sc.data(), s->d_cols, slots * 4, hipMemcpyDeviceToHost));
  CK(dcopy(s, sv.data(), s->d_vals, slots * 8, hipMemcpyDeviceToHost));
  using Hop = PkrHop;
  std::vector<std::vector<Hop>> ul(du), dl(dd);
  std::vector<char> useen(du, 0), dseen(dd, 0);
  std::vector<Hop> lu, ld;
  for (int64_t i = 0; i < dim; i++) {
    const int64_t iw = i / du, iu = i - iw * du, base = sptr[i >> 6] + (i & 63);
    lu.clear();
    ld.clear();
    for (int k = 0; k < cnt[i]; k++) {
      const int64_t q = base + 64 * (int64_t)k;
      const int64_t c = sc[q], cw = c / du, cu = c - cw * du;
      uint64_t bits;
      memcpy(&bits, &sv[q], 8);
      if (cw == iw && cu != iu) lu.push_back({(int32_t)cu, bits});
      else if (cu == iu && cw != iw) ld.push_back({(int32_t)cw, bits});
      else return -1;
    }
    if (!useen[iu]) { ul[iu] = lu; useen[iu] = 1; } else if (ul[iu] != lu) return -1;
    if (!dseen[iw]) { dl[iw] = ld; dseen[iw] = 1; } else if (dl[iw] != ld) return -1;
  }
  int degu = 0, degd = 0;
  for (auto& l : ul) degu = std::max<int>(degu, (int)l.size());
  for (auto& l : dl) degd = std::max<int>(degd, (int)l.size());
  if (pkr_geom(s, du, dd, degu, degd) < 0) return -1;
  pkr_order_up(ul, (int)du, s->pkr_E);
  s->pkr_degu = s->pkr_E;
  CK(pkr_upload(s, ul, s->pkr_degu, du, &s->d_kupc, &s->d_kupv));
  CK(pkr_upload(s, dl, degd, dd, &s->d_kdwc, &s->d_kdwv));
  s->d_kdiag = (const double*)s->d_diag;
  s->pkr_state = 1;
  return 1;
}

// MODE 4 tables of a matrix-free sector: the Kronecker hop tables themselves
// (diagonal generated in-kernel from aup + adw + U, as k_kron).
static int build_pkron_direct(ed_sector* s) {
  if (s->pkr_state && s->pkr_src == 2) return s->pkr_state;
  s->pkr_state = -1;
  s->pkr_src = 2;
  if (s->hc || !s->kron || !s->K.diag_real) return -1;
  const KronHost& K = s->K;
  if (pkr_geom(s, K.dimup, K.dimdw, K.degup, K.degdw) < 0) return -1;
  // up lists from the hop tables ([deg][DimUp], padded with (own column, 0)),
  // reordered for the LDS banks like the stored ones
  const int64_t du = K.dimup;
  std::vector<int32_t> uc((size_t)K.degup * du);
  std::vector<double> uv((size_t)K.degup * du);
  if (K.degup) {
    CK(dcopy(s, uc.data(), K.upc, uc.size() * 4, hipMemcpyDeviceToHost));
    CK(dcopy(s, uv.data(), K.upv, uv.size() * 8, hipMemcpyDeviceToHost));
  }
  std::vector<std::vector<PkrHop>> ul(du);
  for (int64_t r = 0; r < du; r++)
    for (int e = 0; e < K.degup; e++) {
      uint64_t bits;
      memcpy(&bits, &uv[(size_t)e * du + r], 8);
      ul[r].push_back({uc[(size_t)e * du + r], bits});
    }
  pkr_order_up(ul, (int)du, s->pkr_E);
  s->pkr_degu = s->pkr_E;
  CK(pkr_upload(s, ul, s->pkr_degu, du, &s->d_kupc, &s->d_kupv));
  s->d_kdwc = K.dwc;
  s->d_kdwv = (const double*)K.dwv;
  s->d_kdiag = nullptr;
  s->pkr_state = 1;
  return 1;
}

// Returns the persistent mode (0 stored, 1 Kronecker, 2 stored in registers)
// or -1 when the sector does not fit one workgroup's LDS / register budget.
static int64_t persist_lds(const ed_sector* s, int vc, int mode);
// LDS vector rows of a persistent launch: NT * RPT (padding rows stay zero)
static int64_t persist_vrows(const ed_sector* s, int mode, int vc = 0) {
  switch (mode) {
    case 2: return (int64_t)kPRegBlock * s->preg_rpt;
    case 3: return (int64_t)kPRegBlock * s->kreg_rpt;
    case 4: return (int64_t)kPRegBlock * s->pkr_rpt;
    default: return (int64_t)kPBlock * persist_rpt01(s->dim);
  }
}
// ELL words per lane that compile without scratch (-Rpass-analysis=kernel-resource-usage)
static int persist_mode_derive(ed_sector* s, int vc, int path) {
  const int o = s->opts;
  if (o & ED_OPT_NO_PERSIST) return -1;
  const int64_t vs = vc ? 16 : 8;
  // rows per thread beyond which the register-resident p/w arrays spill
  // (-Rpass-analysis: 0-8 B/lane scratch up to 8 real / 5 complex rows)
  const int64_t rpt_max = (vc || s->hc) ? 5 : 8;
  if (s->dim > rpt_max * (int64_t)kPBlock) return -1;
  int64_t lds = ((persist_vrows(s, 0) * vs + 15) & ~(int64_t)15);
  // MODE 4 (Kronecker register layout, real H): c2 2.2 us/step (real
  // vectors); complex vectors in their 1024-thread form
  if (!(o & (ED_OPT_NO_PKRON | ED_OPT_NO_PREG)) &&
      ((path == 0 && !(o & ED_OPT_PERSIST_STORED) && build_pkron_stored(s) > 0) ||
       (path == 2 && build_pkron_direct(s) > 0)) &&
      (vc == 0 || pkr_fits_c512(s->pkr_E, s->pkr_rpt)) &&
      persist_lds(s, vc, 4) <= kLdsBudget)
    return 4;
  // stored: MODE 2 (ELL entries in registers; c2 4.6 us/step) by default.
  // MODE 0 streams the matrix from L2 through one CU (~40-50 GB/s) and is
  // slower than the graph-captured multi-kernel recurrence (c2: 9.8 vs 8.9
  // us/step): opt-in only (ED_OPT_PERSIST_STORED), for coverage
  if (path == 0) {
    if (o & ED_OPT_PERSIST_STORED) return lds <= kLdsBudget ? 0 : -1;
    if (o & ED_OPT_NO_PREG) return -1;
    // MODE 2: dictionary + v + diagonal in LDS; RPT x W words + RPT x (p, w)
    // in registers (512-thread blocks: 256 VGPRs per lane)
    if (s->dim > 10 * (int64_t)kPRegBlock) return -1;
    const int W = build_preg(s);
    if (W < 0) return -1;
    if (s->preg_rpt * W > preg_cap(s->hc, vc)) return -1;
    if (persist_lds(s, vc, 2) > kLdsBudget) return -1;
    return 2;
  }
  if (path == 2 && !(o & ED_OPT_NO_PREG) && s->dim <= 10 * (int64_t)kPRegBlock) {
    // MODE 3: ELL words generated in-kernel from the hop tables
    const KronHost& K = s->K;
    const int deg = K.degup + K.degdw;
    int W = 0;
    for (int w : {8, 12, 14, 16})
      if (!W && deg <= w) W = w;
    const int64_t rpt = (s->dim + kPRegBlock - 1) / kPRegBlock;
    const int RPT = rpt <= 2 ? 2 : rpt <= 4 ? 4 : rpt <= 6 ? 6 : rpt <= 8 ? 8 : 10;
    const int64_t hs = s->hc ? 16 : 8;
    const int64_t dict = ((int64_t)(K.degup * K.dimup + K.degdw * K.dimdw) + 1) * hs;
    const int cap = preg_cap(s->hc, vc);
    const int64_t vr = (int64_t)kPRegBlock * RPT;
    const int64_t l3 = ((dict + 15) & ~(int64_t)15) + ((vr * vs + 15) & ~(int64_t)15) + ((vr * 8 + 15) & ~(int64_t)15);
    if (W && RPT * W <= cap && dict <= (int64_t)kPkOffMask + 1 && l3 <= kLdsBudget && K.diag_real) {
      s->kreg_W = W;
      s->kreg_rpt = RPT;
      return 3;
    }
  }
  if (path == 2) {
    const KronHost& K = s->K;
    const int64_t hs = s->hc ? 16 : 8;
    lds += (K.dimup + K.dimdw) * (hs + 1 + 32) + (int64_t)(K.degup * K.dimup + K.degdw * K.dimdw) * (hs + 4) +
           (int64_t)K.nimp * K.nimp * 8 + 256;
    return lds <= kLdsBudget ? 1 : -1;
  }
  return -1;
}

static int64_t persist_lds(const ed_sector* s, int vc, int mode) {
  const int64_t vs = vc ? 16 : 8, vr = persist_vrows(s, mode, vc);
  int64_t lds = ((vr * vs + 15) & ~(int64_t)15);
  if (mode == 4) {
    // real vectors: slot-major, RPT slots of NT + 1 elements (k_lanc_persist
    // VSLOT); complex vectors: natural order + the down-hop value table
    if (!vc) return (((vr + vr / kPRegBlock) * vs + 15) & ~(int64_t)15);
    return lds + (int64_t)s->pkr_E * s->pkr_dd * 8;
  }
  if (mode == 2) {
    const int64_t hs = s->hc ? 16 : 8;
    return lds + ((vr * 8 + 15) & ~(int64_t)15) + (((int64_t)s->ndict * hs + 15) & ~(int64_t)15);
  }
  if (mode == 3) {
    const int64_t hs = s->hc ? 16 : 8;
    const int64_t dict = ((int64_t)(s->K.degup * s->K.dimup + s->K.degdw * s->K.dimdw) + 1) * hs;
    return lds + ((vr * 8 + 15) & ~(int64_t)15) + ((dict + 15) & ~(int64_t)15);
  }
  if (mode == 1) {
    const KronHost& K = s->K;
    const int64_t hs = s->hc ? 16 : 8;
    auto al = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
    lds += al(K.dimup * hs) + al(K.dimdw * hs) + al((int64_t)K.degup * K.dimup * hs) +
           al((int64_t)K.degdw * K.dimdw * hs) + al((int64_t)K.degup * K.dimup * 4) +
           al((int64_t)K.degdw * K.dimdw * 4) + al(K.dimup) + al(K.dimdw) + al((int64_t)K.nimp * K.nimp * 8);
  }
  return lds;
}

// The mode for (vc, path) under the sector's options, derived once: every
// Lanczos entry point asks on every call, and the answer (with the tables it
// builds) changes only with these three (ed_sector_set_options drops it).
static int persist_mode(ed_sector* s, int vc, int path) {
  auto& c = s->pchoice;
  if (c.vc == vc && c.path == path && c.opts == s->opts) return c.mode;
  c.vc = -1;  // not valid while the tables are rebuilt
  const int mode = persist_mode_derive(s, vc, path);
  c.lds = mode >= 0 ? persist_lds(s, vc, mode) : 0;
  c.mode = mode;
  c.path = path;
  c.opts = s->opts;
  c.vc = vc;
  return mode;
}

static PersistGeom persist_geom(const ed_sector* s) {
  PersistGeom g;
  g.dim = s->dim;
  g.preg_E = s->preg_E;
  g.preg_rpt = s->preg_rpt;
  g.kreg_W = s->kreg_W;
  g.kreg_rpt = s->kreg_rpt;
  g.pkr_E = s->pkr_E;
  g.pkr_rpt = s->pkr_rpt;
  g.device = s->device;
  return g;
}

// Workspace of a batched persistent launch: nb runs on the same H, run b at
// R + b*ldr, P + b*ldp, st + b, alpha/beta + b*ldab.
struct PersistBatch {
  int nb;
  void *R, *P;
  LancState* st;
  double *alpha, *beta;
  int64_t ldr, ldp, ldab;
};

// Launch `niter` persistent iterations.  first=1 starts from the device
// vector v0 (only read; batched: run b at v0 + b*dim), or from R when v0 is
// null.  A first launch needs nothing prepared on the stream: the kernel
// initialises the LancState, beta[0] and, on an early stop, the zeros behind
// the last step.  host_ab: the kernel's one lane stores alpha and beta of each
// step straight into the pinned staging block w.h_ab (alpha | beta at cap + 2;
// device-visible host memory, two 8-B stores per step that nothing waits
// for), so no download of them follows the run.
template <bool VC>
static int persist_iters(ed_sector* s, int mode, bool basis, int niter, int first, hipStream_t st,
                         const PersistBatch* bt = nullptr, const void* v0 = nullptr, bool host_ab = false) {
  LancWS& w = s->ws;
  const int nb = bt ? bt->nb : 1;
  auto fill = [&](auto& r) {
    using RT = std::remove_reference_t<decltype(r)>;
    using HT = std::remove_const_t<std::remove_pointer_t<decltype(r.diag)>>;
    memset(&r, 0, sizeof(RT));
    r.diag = (const HT*)s->d_diag;
    r.sptr = s->d_sptr;
    r.cols = s->d_cols;
    r.vals = (const HT*)s->d_vals;
    r.dim = s->dim;
    r.R = w.R;
    r.v0 = first ? v0 : nullptr;
    r.P = w.P;
    r.st = w.st;
    r.alpha = host_ab ? w.h_ab : w.alpha;
    r.beta = host_ab ? w.h_ab + w.cap + 2 : w.beta;
    r.basis = basis ? w.basis : nullptr;
    r.niter = niter;
    r.first = first;
    r.thresh = s->pthresh;
    r.pk = s->d_pk;
    r.dict = (const HT*)s->d_dict;
    r.ndict = s->ndict;
    r.kupc = s->d_kupc;
    r.kupv = s->d_kupv;
    r.kdwc = s->d_kdwc;
    r.kdwv = s->d_kdwv;
    r.kdiag = s->d_kdiag;
    r.kdu = s->pkr_du;
    r.kdd = s->pkr_dd;
    r.kdegu = s->pkr_degu;
    r.kdegd = s->pkr_degd;
    if (bt) {
      r.R = bt->R;
      r.P = bt->P;
      r.st = bt->st;
      r.alpha = bt->alpha;
      r.beta = bt->beta;
      r.basis = nullptr;
      r.ldr = bt->ldr;
      r.ldp = bt->ldp;
      r.ldab = bt->ldab;
    }
  };
  const auto& pc = s->pchoice;
  const int64_t lds = (pc.vc == (int)VC && pc.mode == mode) ? pc.lds : persist_lds(s, VC, mode);
  if (s->hc) {
    if constexpr (!VC) return fail(ED_ERR_ARG, "complex H needs complex vectors");
    else {
      PersistRun<true> r;
      fill(r);
      if (mode == 1 || mode == 3) r.K = kron_args<true>(s);
      if (mode == 4) return fail(ED_ERR_UNSUPPORTED, "MODE 4 needs real H");
      return persist_launch(true, true, mode, persist_geom(s), &r, lds, st, nb);
    }
  }
  PersistRun<false> r;
  fill(r);
  if (mode == 1 || mode == 3 || (mode == 4 && s->kron)) r.K = kron_args<false>(s);
  return persist_launch(false, VC, mode, persist_geom(s), &r, lds, st, nb);
}

static int persist_set_thresh(ed_sector* s, double thresh, hipStream_t st) {
  // nothing on the stream: the threshold travels in the kernel argument; the
  // first launch initialises the LancState, writes beta[0] = 0 and, when it
  // stops early, the zeros behind its last step (k_lanc_persist)
  (void)st;
  s->pthresh = thresh;
  return ED_OK;
}

// One Lanczos driver for every entry point: persistent one-workgroup kernel
// when the sector fits a CU, graph-captured two-kernel recurrence otherwise.
static int lanc_load_start(ed_sector* s, int vc, const void* v0, bool v0_device);

struct LancDriver {
  ed_sector* s;
  int vc, path, pm;
  bool basis;
  hipStream_t st;
  int start(double thresh) {
    if (pm >= 0) return persist_set_thresh(s, thresh, st);
    return vc ? lanc_start<true>(s, thresh, st) : lanc_start<false>(s, thresh, st);
  }
  // v0 (persistent kernel, first launch): a device start vector read in
  // place; null: the vector lanc_load_start left in ws.R
  int iters(int n, bool first, const void* v0 = nullptr) {
    if (pm >= 0)  // alpha and beta land in the pinned staging block (fetch)
      return vc ? persist_iters<true>(s, pm, basis, n, first ? 1 : 0, st, nullptr, v0, true)
                : persist_iters<false>(s, pm, basis, n, first ? 1 : 0, st, nullptr, v0, true);
    return vc ? lanc_iters<true>(s, path, basis, n, st) : lanc_iters<false>(s, path, basis, n, st);
  }
  // alpha[0, na), beta[0, nb) and the LancState of the run so far, behind one
  // host sync.  Persistent kernel: alpha and beta are already in host memory
  // (the staging block), only the state is downloaded.
  int fetch(double* a, int na, double* b, int nb, LancState* hs) {
    LancWS& w = s->ws;
    if (pm < 0) {
      HIPCK(hipMemcpyAsync(a, w.alpha, (size_t)na * 8, hipMemcpyDeviceToHost, st));
      HIPCK(hipMemcpyAsync(b, w.beta, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipMemcpyAsync(hs, w.st, sizeof(*hs), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (pm >= 0) {
      memcpy(a, w.h_ab, (size_t)na * 8);
      memcpy(b, w.h_ab + w.cap + 2, (size_t)nb * 8);
    }
    return ED_OK;
  }
  // Start vector of a run: a device vector stays where it is when the
  // persistent kernel takes the run (returned for iters); otherwise it is
  // loaded into ws.R
  int load(const void* v0, bool v0_device, const void** inplace) {
    *inplace = nullptr;
    if (pm >= 0 && v0 && v0_device) {
      *inplace = v0;
      return ED_OK;
    }
    return lanc_load_start(s, vc, v0, v0_device);
  }
};

static int make_driver(ed_sector* s, int vtype, bool basis, LancDriver* d) {
  CK(whole_only(s));
  d->s = s;
  d->vc = vtype ? 1 : 0;
  if (d->vc == 0 && s->hc) return fail(ED_ERR_ARG, "complex H needs vtype=1");
  d->path = resolve_path(s, -1);
  d->pm = persist_mode(s, d->vc, d->path);
  d->basis = basis;
  d->st = s->stream;
  return ED_OK;
}

static int lanc_load_start(ed_sector* s, int vc, const void* v0, bool v0_device) {
  const size_t vs = vc ? 16 : 8;
  if (v0) {
    HIPCK(hipMemcpyAsync(s->ws.R, v0, s->dim * vs,
                         v0_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
  } else {
    hipLaunchKernelGGL(k_default_start, dim3(grid_for(s->dim * (vc ? 2 : 1))), dim3(kBlock), 0,
                       s->stream, (double*)s->ws.R, s->dim * (vc ? 2 : 1));
    HIPCK(hipGetLastError());
  }
  return ED_OK;
}

extern "C" {

// Fixed-length run from a device start vector (benchmark entry point).
int ed_sector_lanc_run(ed_sector* s, int32_t vtype, const void* v0_dev, int32_t niter,
                       double* alfa, double* beta, float* ms, void* stream) {
  (void)stream;
  if (!s || niter < 1) return fail(ED_ERR_ARG, "bad args");
  HIPCK(hipSetDevice(s->device));
  LancDriver d;
  CK(make_driver(s, vtype, false, &d));
  CK(lanc_prepare(s, d.vc, niter, false, 0));
  // persistent kernel: the stream gets the two event records and one kernel
  // (the start vector is read in place, nothing is cleared, alpha and beta
  // land in the staging block)
  const void* v0p = nullptr;
  CK(d.load(v0_dev, true, &v0p));
  LancWS& w = s->ws;
  for (hipEvent_t& e : w.ev)
    if (!e) HIPCK(hipEventCreate(&e));
  hipEvent_t e0 = w.ev[0], e1 = w.ev[1];
  int rc = d.start(1e-300);
  if (rc == ED_OK) {
    HIPCK(hipEventRecord(e0, d.st));
    rc = d.iters(niter, true, v0p);
    HIPCK(hipEventRecord(e1, d.st));
  }
  // one host sync for the run; the multi-kernel recurrence downloads
  // alpha | beta into the staging block, the persistent kernel wrote them there
  const size_t nab = (size_t)w.cap + 2 + niter;
  if (rc == ED_OK && (alfa || beta) && d.pm < 0)
    HIPCK(hipMemcpyAsync(w.h_ab, w.alpha, nab * sizeof(double), hipMemcpyDeviceToHost, d.st));
  HIPCK(hipStreamSynchronize(d.st));
  CK(rc);
  if (alfa) memcpy(alfa, w.h_ab, niter * sizeof(double));
  if (beta) memcpy(beta, w.h_ab + w.cap + 2, niter * sizeof(double));
  if (ms) HIPCK(hipEventElapsedTime(ms, e0, e1));
  return ED_OK;
}

// lanczos_plain_tridiag_c: alanc(iter)=a; if(iter<nitermax)blanc(iter+1)=b; exit if |b|<thr.
// The n steps of one run, as the caller's alfa[nitermax] / beta[nitermax].
static void unpack_tridiag(const double* a, const double* b, int n, int nitermax, double* alfa, double* beta,
                           int32_t* nlanc) {
  for (int q = 0; q < nitermax; q++) {
    alfa[q] = q < n ? a[q] : 0.0;
    beta[q] = (q >= 1 && q <= n) ? b[q] : 0.0;
  }
  beta[0] = 0.0;
  if (nlanc) *nlanc = n;
}

// One run of at most nitermax steps on the prepared workspace, from v0 (host
// or device memory; null: the default start vector)
static int lanc_tridiag_one(LancDriver& d, const void* v0, bool v0_device, int nitermax, double threshold,
                            double* alfa, double* beta, int32_t* nlanc) {
  const void* v0p = nullptr;
  CK(d.load(v0, v0_device, &v0p));
  CK(d.start(threshold));
  CK(d.iters(nitermax, true, v0p));
  std::vector<double> a(nitermax + 1), b(nitermax + 2);
  LancState hs;
  CK(d.fetch(a.data(), nitermax, b.data(), nitermax + 1, &hs));
  unpack_tridiag(a.data(), b.data(), hs.iter, nitermax, alfa, beta, nlanc);
  return ED_OK;
}

int ed_sector_lanc_tridiag(ed_sector* s, int32_t vtype, const void* v0, int32_t nitermax,
                           double threshold, double* alfa, double* beta, int32_t* nlanc) {
  if (!s || !alfa || !beta || nitermax < 1) return fail(ED_ERR_ARG, "bad args");
  HIPCK(hipSetDevice(s->device));
  LancDriver d;
  CK(make_driver(s, vtype, false, &d));
  CK(lanc_prepare(s, d.vc, nitermax, false, 0));
  return lanc_tridiag_one(d, v0, false, nitermax, threshold, alfa, beta, nlanc);
}

// sp_lanc_tridiag for nseed start vectors on one sector (GF seeds of one
// target sector: ED_GF_NORMAL.f90:180-193, ED_GF_NONSU2.f90:343-886).  When
// the sector runs the persistent one-workgroup recurrence, all seeds go in
// ONE launch, one workgroup each (same per-workgroup code as a single run:
// identical alpha/beta); otherwise the seeds run one after the other.
int ed_sector_lanc_tridiag_batch(ed_sector* s, int32_t vtype, int32_t nseed, const void* v0_dev,
                                 int32_t nitermax, double threshold, double* alfa, double* beta,
                                 int32_t* nlanc) {
  if (!s || !v0_dev || !alfa || !beta || nitermax < 1 || nseed < 1) return fail(ED_ERR_ARG, "bad args");
  HIPCK(hipSetDevice(s->device));
  LancDriver d;
  CK(make_driver(s, vtype, false, &d));
  const size_t vs = d.vc ? 16 : 8;
  if (d.pm < 0 || (s->opts & ED_OPT_NO_BATCH)) {
    CK(lanc_prepare(s, d.vc, nitermax, false, 0));
    for (int k = 0; k < nseed; k++)
      CK(lanc_tridiag_one(d, (const unsigned char*)v0_dev + (size_t)k * s->dim * vs, true, nitermax, threshold,
                          alfa + (size_t)k * nitermax, beta + (size_t)k * nitermax, nlanc ? nlanc + k : nullptr));
    return ED_OK;
  }
  CK(lanc_prepare(s, d.vc, nitermax, false, 0));  // register tables / dictionaries of the persistent mode
  PersistBatch bt;
  bt.nb = nseed;
  bt.ldr = s->dim;
  bt.ldp = (int64_t)p_rows(s);
  bt.ldab = 2 * ((int64_t)nitermax + 2);
  hipStream_t st = d.st;
  // freed on the stream at every return, an allocation failure's included
  DevFree fR{nullptr, st}, fP{nullptr, st}, fab{nullptr, st}, fsts{nullptr, st};
  HIPCK(hipMallocAsync(&fR.p, (size_t)nseed * bt.ldr * vs, st));
  HIPCK(hipMallocAsync(&fP.p, (size_t)nseed * bt.ldp * vs, st));
  HIPCK(hipMallocAsync(&fab.p, (size_t)nseed * bt.ldab * 8, st));
  HIPCK(hipMallocAsync(&fsts.p, (size_t)nseed * sizeof(LancState), st));
  void *const ab = fab.p, *const sts = fsts.p;
  bt.R = fR.p;
  bt.P = fP.p;
  bt.st = (LancState*)sts;
  bt.alpha = (double*)ab;
  bt.beta = (double*)ab + nitermax + 2;
  s->pthresh = threshold;
  // one kernel: every run reads its seed in place (run b at v0_dev + b*dim,
  // ldr = dim), starts from p = 0 and initialises its own LancState, beta[0]
  // and, on an early stop, its alpha / beta tail
  int rc = with_vc(d.vc, [&](auto c) {
    return persist_iters<decltype(c)::value>(s, d.pm, false, nitermax, 1, st, &bt, v0_dev);
  });
  std::vector<double> hab((size_t)nseed * bt.ldab);
  std::vector<LancState> hst(nseed);
  if (rc == ED_OK) {
    HIPCK(hipMemcpyAsync(hab.data(), ab, hab.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(hst.data(), sts, nseed * sizeof(LancState), hipMemcpyDeviceToHost, st));
  }
  HIPCK(hipStreamSynchronize(st));
  CK(rc);
  for (int k = 0; k < nseed; k++) {
    // a run that never broke down ends with st->iter = nitermax
    const double* a = hab.data() + (size_t)k * bt.ldab;
    unpack_tridiag(a, a + nitermax + 2, hst[k].iter, nitermax, alfa + (size_t)k * nitermax,
                   beta + (size_t)k * nitermax, nlanc ? nlanc + k : nullptr);
  }
  return ED_OK;
}

}  // extern "C"

// ---------------------------------------------- lockstep multi-vector runs
// Workspace of one group of at most `width` runs (ed_multi.hpp): the
// row-interleaved blocks R, P, W, one LancState per run, the block partials
// of a pass ([width][np]) and alpha | beta of every run (run v at ab + v*ldab,
// beta nitermax + 2 behind alpha, as PersistBatch lays them out).
struct LockWS {
  void *R, *P, *W;
  LancState* st;
  double *partials, *ab;
  int64_t ldab;
  int np;
};
// grid of the element-wise passes (init, part B): enough blocks to fill the
// chip; their partials are summed by one block per run
static constexpr int kLockPassGrid = 4096;
static int lock_pass_grid(int64_t n) { return std::min(grid_for(n), kLockPassGrid); }

// nitermax steps of NV runs in lockstep from seeds (NV vectors of dim, the
// batch entry's layout).  One step: block H·X with the Lanczos epilogue, its
// finish, part B, its finish — four launches in stream order (a capture of
// them would have no parallel branch; they are launched directly because the
// workspace is allocated per call, and a captured graph bakes its pointers in).
template <bool VC, int NV>
static int lockstep_group(ed_sector* s, const LockWS& w, const void* seeds, int nitermax, double thresh,
                          hipStream_t st) {
  using V = val_t<VC>;
  const int64_t n = s->dim * NV, boff = (int64_t)nitermax + 2;
  const int g0 = lock_pass_grid(s->dim), g1 = hxv_mv_blocks(s), g2 = lock_pass_grid(n);
  HIPCK(hipMemsetAsync(w.ab, 0, (size_t)NV * w.ldab * sizeof(double), st));  // alpha | beta
  hipLaunchKernelGGL((k_lanc_init_mv<VC, NV>), dim3(g0), dim3(kBlock), 0, st, (const V*)seeds, (V*)w.R, (V*)w.P,
                     s->dim, w.partials);
  hipLaunchKernelGGL(k_lanc_fin_mv<0>, dim3(NV), dim3(kBlock), 0, st, w.partials, g0, w.st, w.ab, w.ldab, boff, thresh);
  HIPCK(hipGetLastError());
  EpiLancAMV<VC, NV> e{};
  e.st = w.st;
  e.P = (V*)w.P;
  e.W = (V*)w.W;
  e.partials = w.partials;
  for (int k = 0; k < nitermax; k++) {
    CK((launch_hxv_mv<VC, NV>(s, w.R, e, st)));
    hipLaunchKernelGGL(k_lanc_fin_mv<1>, dim3(NV), dim3(kBlock), 0, st, w.partials, g1, w.st, w.ab, w.ldab, boff, thresh);
    hipLaunchKernelGGL((k_lanc_b_mv<VC, NV>), dim3(g2), dim3(kBlock), 0, st, (const V*)w.W, (const V*)w.P, (V*)w.R, n,
                       w.st, w.partials);
    hipLaunchKernelGGL(k_lanc_fin_mv<2>, dim3(NV), dim3(kBlock), 0, st, w.partials, g2, w.st, w.ab, w.ldab, boff, thresh);
  }
  HIPCK(hipGetLastError());
  return ED_OK;
}

template <bool VC>
static int lockstep_group_nv(ed_sector* s, int nv, const LockWS& w, const void* seeds, int nitermax, double thresh,
                             hipStream_t st) {
  switch (nv) {
    case 8: return lockstep_group<VC, 8>(s, w, seeds, nitermax, thresh, st);
    case 4: return lockstep_group<VC, 4>(s, w, seeds, nitermax, thresh, st);
    case 2: return lockstep_group<VC, 2>(s, w, seeds, nitermax, thresh, st);
    default: return lockstep_group<VC, 1>(s, w, seeds, nitermax, thresh, st);
  }
}

extern "C" {

// sp_lanc_tridiag (.repo/PLAIN_LANCZOS.f90:87-118) for nseed start vectors
// that advance together: the seeds are cut into groups of 8, 4, 2, 1
// (ed_lockstep_groups.hpp) and each group's vectors are interleaved by row, so
// one pass over the stored H (k_spmv_mv, ed_multi.hpp) serves the whole group.
// Per run the arithmetic is lanc_iter's; the two dot products of a step are
// summed over other block shapes, so alpha and beta agree with
// ed_sector_lanc_tridiag_batch to rounding, not bit for bit.
int ed_sector_lanc_tridiag_lockstep(ed_sector* s, int32_t vtype, int32_t nseed, const void* v0_dev,
                                    int32_t nitermax, double threshold, double* alfa, double* beta,
                                    int32_t* nlanc) {
  if (nseed < 1) return fail(ED_ERR_ARG, "nseed must be positive");
  if (nitermax < 1) return fail(ED_ERR_ARG, "nitermax must be positive");
  if (vtype != 0 && vtype != 1) return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
  if (!s || !v0_dev || !alfa || !beta) return fail(ED_ERR_ARG, "null");
  if (vtype == 0 && s->hc) return fail(ED_ERR_ARG, "complex H needs vtype=1");
  const size_t vs = vtype ? 16 : 8;
  if ((uintptr_t)v0_dev & (vs - 1)) return fail(ED_ERR_ARG, "v0_dev must be aligned to its element type");
  CK(mv_sector_check(s));
  HIPCK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  std::vector<int> first(lockstep_max_groups(nseed)), width(first.size());
  const int ngroup = lockstep_groups(nseed, first.data(), width.data());
  // one group's workspace, sized by the widest (the first); the later groups reuse it
  const int w0 = width[0];
  LockWS w;
  w.ldab = 2 * ((int64_t)nitermax + 2);
  w.np = std::max(hxv_mv_blocks(s), lock_pass_grid(s->dim * w0));
  // freed on the stream at every return, an allocation failure's included
  DevFree fR{nullptr, st}, fP{nullptr, st}, fW{nullptr, st}, fst{nullptr, st}, fpart{nullptr, st}, fab{nullptr, st};
  HIPCK(hipMallocAsync(&fR.p, (size_t)s->dim * w0 * vs, st));
  HIPCK(hipMallocAsync(&fP.p, (size_t)s->dim * w0 * vs, st));
  HIPCK(hipMallocAsync(&fW.p, (size_t)s->dim * w0 * vs, st));
  HIPCK(hipMallocAsync(&fst.p, (size_t)w0 * sizeof(LancState), st));
  HIPCK(hipMallocAsync(&fpart.p, (size_t)w0 * w.np * sizeof(double), st));
  HIPCK(hipMallocAsync(&fab.p, (size_t)w0 * w.ldab * sizeof(double), st));
  w.R = fR.p;
  w.P = fP.p;
  w.W = fW.p;
  w.st = (LancState*)fst.p;
  w.partials = (double*)fpart.p;
  w.ab = (double*)fab.p;
  std::vector<double> hab((size_t)nseed * w.ldab);
  std::vector<LancState> hst(nseed);
  int rc = ED_OK;
  for (int g = 0; g < ngroup && rc == ED_OK; g++) {
    const void* seeds = (const unsigned char*)v0_dev + (size_t)first[g] * s->dim * vs;
    rc = with_vc(vtype != 0, [&](auto c) {
      return lockstep_group_nv<decltype(c)::value>(s, width[g], w, seeds, nitermax, threshold, st);
    });
    if (rc != ED_OK) break;
    // (stream order: the copies are complete before the next group clears the block)
    hipError_t e1 = hipMemcpyAsync(hab.data() + (size_t)first[g] * w.ldab, w.ab, (size_t)width[g] * w.ldab * 8,
                                   hipMemcpyDeviceToHost, st);
    hipError_t e2 = hipMemcpyAsync(hst.data() + first[g], w.st, (size_t)width[g] * sizeof(LancState),
                                   hipMemcpyDeviceToHost, st);
    if (e1 != hipSuccess || e2 != hipSuccess)
      rc = fail(ED_ERR_HIP, std::string("lockstep download -> ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  }
  HIPCK(hipStreamSynchronize(st));
  CK(rc);
  for (int k = 0; k < nseed; k++) {
    const double* a = hab.data() + (size_t)k * w.ldab;
    unpack_tridiag(a, a + nitermax + 2, hst[k].iter, nitermax, alfa + (size_t)k * nitermax,
                   beta + (size_t)k * nitermax, nlanc ? nlanc + k : nullptr);
  }
  return ED_OK;
}

int ed_sector_lanc_tridiag_dev(ed_sector* s, int32_t vtype, const void* v0_dev, int32_t nitermax,
                               double threshold, double* alfa, double* beta, int32_t* nlanc) {
  if (!s || !alfa || !beta || !v0_dev || nitermax < 1) return fail(ED_ERR_ARG, "bad args");
  HIPCK(hipSetDevice(s->device));
  LancDriver d;
  CK(make_driver(s, vtype, false, &d));
  CK(lanc_prepare(s, d.vc, nitermax, false, 0));
  // v0_dev must be complete when this is called (the caller synchronises the
  // stream that produced it): no device-wide sync, which would fail while
  // another host thread captures a graph on its own sector stream
  return lanc_tridiag_one(d, v0_dev, true, nitermax, threshold, alfa, beta, nlanc);
}

int ed_sector_lanc_eigh(ed_sector* s, int32_t vtype, const void* v0, int32_t nitermax,
                        double threshold, int32_t ncheck, double* egs, void* vect,
                        int32_t* nlanc) {
  if (!s || !egs || nitermax < 1) return fail(ED_ERR_ARG, "bad args");
  if (ncheck < 1) ncheck = 10;
  HIPCK(hipSetDevice(s->device));
  const int vc = vtype ? 1 : 0;
  const size_t vs = vc ? 16 : 8;
  // keep the Krylov basis when it fits in 1/4 of free memory (no second pass)
  size_t fr = 0, tot = 0;
  HIPCK(hipMemGetInfo(&fr, &tot));
  const bool keep = vect && ((double)nitermax * s->dim * vs < 0.25 * (double)fr);
  LancDriver d;
  CK(make_driver(s, vtype, keep, &d));
  CK(lanc_prepare(s, vc, nitermax, keep, keep ? nitermax : 0));
  CK(lanc_load_start(s, vc, v0, false));
  CK(d.start(threshold));
  // lanczos_plain_c convergence test, evaluated on the host between chunks
  std::vector<double> a(nitermax + 2, 0.0), b(nitermax + 2, 0.0), esave;
  int done_iters = 0, nl = 0;
  bool stop = false;
  const int chunk = d.pm >= 0 ? 64 : 32;
  while (!stop && done_iters < nitermax) {
    int n = std::min(chunk, nitermax - done_iters);
    const int expected = done_iters + n;
    CK(d.iters(n, done_iters == 0));
    LancState hs;
    CK(d.fetch(a.data(), nitermax, b.data(), nitermax + 1, &hs));
    int have = hs.iter;
    for (int it = done_iters + 1; it <= have && !stop; it++) {
      // iteration `it`: a = a[it-1], b = b[it]
      if (fabs(b[it]) < threshold) { stop = true; break; }
      nl = it;
      if (nl >= ncheck) {
        double e0 = lowest_ritz(a, b, nl);
        esave.push_back(e0);
        if (esave.size() >= 2 && fabs(esave.back() - esave[esave.size() - 2]) <= threshold) stop = true;
      }
    }
    if (hs.done) stop = true;
    if (have < expected && !hs.done) return fail(ED_ERR_STATE, "Lanczos iteration count mismatch");
    done_iters = have;
  }
  if (nl == 0) {
    LancState hs;
    CK(dcopy(s, &hs, s->ws.st, sizeof(hs), hipMemcpyDeviceToHost));
    char msg[256];
    snprintf(msg, sizeof msg,
             "Lanczos made no step: iter=%d done=%d beta0=%g b[1]=%g a[0]=%g path=%d pm=%d keep=%d",
             hs.iter, hs.done, hs.beta, b[1], a[0], d.path, d.pm, (int)keep);
    return fail(ED_ERR_STATE, msg);
  }
  // Ritz value and vector of the truncated tridiagonal (nl iterations)
  std::vector<double> dg(a.begin(), a.begin() + nl), e(nl, 0.0), z((size_t)nl * nl, 0.0);
  for (int q = 1; q < nl; q++) e[q] = b[q];
  for (int q = 0; q < nl; q++) z[q + (size_t)nl * q] = 1.0;
  if (nl > 0) tql2(nl, dg.data(), e.data(), z.data());
  *egs = nl > 0 ? dg[0] : 0.0;
  if (nlanc) *nlanc = nl;
  if (vect && nl > 0) {
    LancWS& w = s->ws;
    HIPCK(hipMemcpyAsync(w.z, z.data(), nl * 8, hipMemcpyHostToDevice, s->stream));  // Z(:,1)
    RedSlot slot{w.partials, w.counter + 2};
    CK(with_vc(vc, [&](auto c) -> int {
      constexpr bool VC = decltype(c)::value;
      using V = val_t<VC>;
      if (keep) {
        hipLaunchKernelGGL(k_ritz<VC>, dim3(grid_once(s->dim)), dim3(kBlock), 0, s->stream,
                           (const V*)w.basis, w.z, nl, s->dim, (V*)w.Y, w.st, slot);
      } else {
        // second pass as lanczos_plain_c (:374-381): rerun the recurrence, y += Z(it,1) v_it
        // (multi-kernel recurrence: its P buffer holds v_it after each step)
        HIPCK(hipMemsetAsync(w.Y, 0, s->dim * vs, s->stream));
        CK(lanc_load_start(s, vc, v0, false));
        CK(lanc_start<VC>(s, threshold, s->stream));
        for (int it = 0; it < nl; it++) {
          CK((lanc_iter<VC>(s, d.path, false, s->stream)));
          hipLaunchKernelGGL(k_axpy_p<VC>, dim3(grid_for(s->dim)), dim3(kBlock), 0, s->stream,
                             (const V*)w.P, w.z, it, s->dim, (V*)w.Y);
        }
        hipLaunchKernelGGL(k_norm<VC>, dim3(grid_once(s->dim)), dim3(kBlock), 0, s->stream,
                           (const V*)w.Y, s->dim, w.st, slot);
      }
      hipLaunchKernelGGL(k_scale_tmp<VC>, dim3(grid_for(s->dim)), dim3(kBlock), 0, s->stream,
                         (V*)w.Y, s->dim, w.st);
      return ED_OK;
    }));
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(vect, w.Y, s->dim * vs, hipMemcpyDefault, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
  }
  return ED_OK;
}

int ed_sector_lanc_mode(ed_sector* s, int32_t vtype, int32_t path) {
  if (!s) {
    fail(ED_ERR_ARG, "null");
    return -2;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -2;
  return persist_mode(s, vtype ? 1 : 0, resolve_path(s, path));
}

// The k_lanc_persist instantiation behind that mode: the template values
// persist_launch (ed_persist_launch.hpp) dispatches on, read from the fields
// persist_mode() and persist_geom() hold.  Nothing is chosen here.
int ed_sector_lanc_geom(ed_sector* s, int32_t vtype, int32_t path, int32_t geom[6]) {
  if (!s || !geom) return fail(ED_ERR_ARG, "null");
  const int vc = vtype ? 1 : 0;
  if (vc == 0 && s->hc) return fail(ED_ERR_ARG, "complex H needs vtype=1");
  HIPCK(hipSetDevice(s->device));
  const int mode = persist_mode(s, vc, resolve_path(s, path));
  const PersistGeom g = persist_geom(s);
  for (int k = 0; k < 6; k++) geom[k] = 0;
  geom[0] = mode;
  geom[5] = s->hc ? 1 : 0;
  if (mode < 0) return ED_OK;
  geom[1] = mode >= 2 ? kPRegBlock : kPBlock;
  geom[2] = mode == 2 ? g.preg_rpt : mode == 3 ? g.kreg_rpt : mode == 4 ? g.pkr_rpt : persist_rpt01(g.dim);
  geom[3] = mode == 2 ? g.preg_E : mode == 3 ? g.kreg_W : mode == 4 ? g.pkr_E : 1;
  geom[4] = (int32_t)s->pchoice.lds;
  return ED_OK;
}

}  // extern "C"
