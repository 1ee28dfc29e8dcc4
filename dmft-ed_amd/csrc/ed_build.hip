// ed_build.hip — the H builders of a sector (ed_sector.hpp): the basis map,
// the stored SELL-64 matrix with its packed, two-segment and fused re-lays,
// the generic matrix-free tables (k_direct) and the Kronecker tables.
// Reached from sector_create (ed_lib.hip) and, for the k_direct tables on
// first use of path 1, through ensure_direct.
#include "ed_sector.hpp"
#include "ed_build_kernels.hpp"

using namespace edg;

// The basis H%map of the sector from its tables, on the sector's stream
int build_map(ed_sector* s) {
  int64_t* bo;
  uint32_t *bi, *bp;
  int32_t *nn, *ps;
  CK(upload(s, &bo, s->T.blk_off));
  CK(upload(s, &bi, s->T.blk_idw));
  CK(upload(s, &nn, s->T.need_cls));
  CK(upload(s, &bp, s->T.by_cls));
  CK(upload(s, &ps, s->T.cls_start));
  CK(dalloc_t(s, &s->d_map, s->dim));
  hipLaunchKernelGGL(k_build_map, dim3(grid_for(s->dim)), dim3(kBlock), 0, s->stream, bo, bi,
                     (int)s->T.blk_idw.size(), nn, bp, ps, s->T.ns, s->dim, s->d_map);
  if (hipGetLastError() != hipSuccess) return fail(ED_ERR_HIP, "k_build_map launch");
  return ED_OK;
}

// ---------------------------------------------------------- stored build
// Dictionary of the distinct off-diagonal values (device hash of bit
// patterns); when there are at most 256, pack every SELL slot into one word.
static int build_pack(ed_sector* s) {
  const int64_t slots = s->padded;
  if (slots == 0) return ED_OK;
  const bool hc = s->hc;
  const int hw = hc ? 2 : 1;
  unsigned long long* table;
  unsigned int* ovf;
  uint8_t* tidx;
  double2* reps = nullptr;
  HIPCK(hipMallocAsync((void**)&table, kDictTable * 8, s->stream));
  HIPCK(hipMallocAsync((void**)&ovf, 4, s->stream));
  HIPCK(hipMallocAsync((void**)&tidx, kDictTable, s->stream));
  if (hc) HIPCK(hipMallocAsync((void**)&reps, kDictTable * 16, s->stream));
  auto cleanup = [&]() {
    (void)hipFreeAsync(table, s->stream);
    (void)hipFreeAsync(ovf, s->stream);
    (void)hipFreeAsync(tidx, s->stream);
    if (reps) (void)hipFreeAsync(reps, s->stream);
  };
  HIPCK(hipMemsetAsync(table, 0xFF, kDictTable * 8, s->stream));
  HIPCK(hipMemsetAsync(ovf, 0, 4, s->stream));
  if (hc)
    hipLaunchKernelGGL(k_dict_insert_c, dim3(grid_for(slots)), dim3(kBlock), 0, s->stream,
                       (const double2*)s->d_vals, slots, table, reps, ovf);
  else
    hipLaunchKernelGGL(k_dict_insert, dim3(grid_for(slots)), dim3(kBlock), 0, s->stream,
                       (const double*)s->d_vals, slots, table, ovf);
  HIPCK(hipGetLastError());
  std::vector<unsigned long long> ht(kDictTable);
  std::vector<double> hr(hc ? 2 * kDictTable : 0);
  unsigned int hov = 0;
  HIPCK(hipMemcpyAsync(ht.data(), table, kDictTable * 8, hipMemcpyDeviceToHost, s->stream));
  if (hc) HIPCK(hipMemcpyAsync(hr.data(), reps, kDictTable * 16, hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipMemcpyAsync(&hov, ovf, 4, hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  std::vector<uint8_t> ti(kDictTable, 0);
  std::vector<double> dict;
  for (int h = 0; h < kDictTable && !hov; h++) {
    if (ht[h] == kDictEmpty) continue;
    if (dict.size() == (size_t)256 * hw) {
      hov = 1;
      break;
    }
    ti[h] = (uint8_t)(dict.size() / hw);
    if (hc) {
      dict.push_back(hr[2 * h]);
      dict.push_back(hr[2 * h + 1]);
    } else {
      double v;
      memcpy(&v, &ht[h], 8);
      dict.push_back(v);
    }
  }
  if (hov) {
    cleanup();
    return ED_OK;  // too many distinct values: the plain SELL path serves
  }
  uint32_t* words = nullptr;
  void* pd = nullptr;
  CK(dalloc(s, &pd, 256 * 8 * hw));
  CK(dalloc(s, (void**)&words, slots * 4));
  HIPCK(hipMemsetAsync(pd, 0, 256 * 8 * hw, s->stream));
  HIPCK(hipMemcpyAsync(pd, dict.data(), dict.size() * 8, hipMemcpyHostToDevice, s->stream));
  HIPCK(hipMemcpyAsync(tidx, ti.data(), kDictTable, hipMemcpyHostToDevice, s->stream));
  if (hc)
    hipLaunchKernelGGL(k_dict_pack_c, dim3(grid_for(slots)), dim3(kBlock), 0, s->stream, s->d_cols,
                       (const double2*)s->d_vals, slots, table, reps, tidx, words, ovf);
  else
    hipLaunchKernelGGL(k_dict_pack, dim3(grid_for(slots)), dim3(kBlock), 0, s->stream, s->d_cols,
                       (const double*)s->d_vals, slots, table, tidx, words);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(&hov, ovf, 4, hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  cleanup();
  if (hov) {  // a 64-bit key collision between two complex values: keep the plain path
    dfree(s, &pd, 256 * 8 * hw);
    dfree(s, (void**)&words, slots * 4);
    return ED_OK;
  }
  s->d_pdict = pd;
  s->d_words = words;
  s->npdict = (int)(dict.size() / hw);
  return ED_OK;
}

// ---------------------------------------------------- two-segment stored H
// (ed_split.hpp).  Built for whole packed sectors whose stored matrix does
// not fit the 256 MB Infinity Cache (the sectors whose one-pass kernel pays
// the down-spin re-gathers from HBM).
static int build_split(ed_sector* s) {
  const int64_t dim = s->dim, ns = s->nslice;
  const int hw = s->hc ? 2 : 1;
  const int nsp = s->Mh.ns;
  // the dictionary's zero (padding slots); appended when absent
  std::vector<double> dict(256 * hw);
  CK(dcopy(s, dict.data(), s->d_pdict, dict.size() * 8, hipMemcpyDeviceToHost));
  int z = -1;
  for (int k = 0; k < s->npdict && z < 0; k++) {
    bool zero = true;
    for (int h = 0; h < hw; h++) zero = zero && dict[k * hw + h] == 0.0 && !std::signbit(dict[k * hw + h]);
    if (zero) z = k;
  }
  if (z < 0) {
    if (s->npdict >= 256) return ED_OK;  // no room for a zero: the one-pass kernel serves
    z = s->npdict++;
    HIPCK(hipMemsetAsync((double*)s->d_pdict + (size_t)z * hw, 0, 8 * hw, s->stream));
  }
  const uint32_t zpad = (uint32_t)z << kPackShift;
  // ---- segment A: counts, slice widths, offsets, fill
  uint16_t* na;
  int32_t* width;
  int64_t *bsum, *total;
  int* farmax;
  const int64_t nb = (ns + 1023) / 1024;
  HIPCK(hipMallocAsync((void**)&na, dim * sizeof(uint16_t), s->stream));
  HIPCK(hipMallocAsync((void**)&width, ns * sizeof(int32_t), s->stream));
  HIPCK(hipMallocAsync((void**)&bsum, std::max<int64_t>(nb, 1) * sizeof(int64_t), s->stream));
  HIPCK(hipMallocAsync((void**)&total, sizeof(int64_t), s->stream));
  HIPCK(hipMallocAsync((void**)&farmax, sizeof(int), s->stream));
  auto scratch_free = [&]() {
    (void)hipFreeAsync(na, s->stream);
    (void)hipFreeAsync(width, s->stream);
    (void)hipFreeAsync(bsum, s->stream);
    (void)hipFreeAsync(total, s->stream);
    (void)hipFreeAsync(farmax, s->stream);
  };
  HIPCK(hipMemsetAsync(farmax, 0, sizeof(int), s->stream));
  hipLaunchKernelGGL(k_split_count_a, dim3(grid_for(ns * 64)), dim3(kBlock), 0, s->stream, s->d_sptr, s->d_words,
                     s->d_cnt, s->d_map, nsp, dim, ns, na, width, farmax);
  HIPCK(hipGetLastError());
  int hfar = 0;
  HIPCK(hipMemcpyAsync(&hfar, farmax, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  if (hfar > kSplitFarMax) {
    scratch_free();
    return ED_OK;  // rows with more cross-block elements than the build stages: one-pass
  }
  // cross-block elements = nnz - dim - sum(nA) (the U entries cover nfar_u of them)
  unsigned long long sumA = 0;
  {
    unsigned long long* dn;
    HIPCK(hipMallocAsync((void**)&dn, sizeof(unsigned long long), s->stream));
    HIPCK(hipMemsetAsync(dn, 0, sizeof(unsigned long long), s->stream));
    hipLaunchKernelGGL(k_sum_u16, dim3(grid_once(dim)), dim3(kBlock), 0, s->stream, na, dim, dn);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(&sumA, dn, sizeof(sumA), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    (void)hipFreeAsync(dn, s->stream);
  }
  const int64_t nfar = s->nnz - dim - (int64_t)sumA;
  CK(dalloc_t(s, &s->d_sptrA, ns + 1));
  hipLaunchKernelGGL(k_scan_blocks, dim3((unsigned)nb), dim3(1024), 0, s->stream, width, ns, s->d_sptrA, bsum);
  hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(64), 0, s->stream, bsum, nb, total);
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(1024), 0, s->stream, s->d_sptrA, ns, bsum, total);
  HIPCK(hipGetLastError());
  int64_t slotsA = 0;
  HIPCK(hipMemcpyAsync(&slotsA, total, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  s->paddedA = slotsA;
  {
    std::vector<int64_t> hp(ns + 1);
    CK(dcopy(s, hp.data(), s->d_sptrA, (ns + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    int wm = 0;
    int wn = 1 << 30;
    for (int64_t q = 0; q < ns; q++) {
      wm = std::max(wm, (int)((hp[q + 1] - hp[q]) >> 6));
      wn = std::min(wn, (int)((hp[q + 1] - hp[q]) >> 6));
    }
    s->wA_max = wm;
    s->wA_min = wn;
  }
  CK(dalloc_t(s, &s->d_wordsA, std::max<int64_t>(slotsA, 1)));
  hipLaunchKernelGGL(k_split_fill_a, dim3(grid_for(ns * 64)), dim3(kBlock), 0, s->stream, s->d_sptr, s->d_words,
                     s->d_cnt, s->d_map, nsp, dim, ns, s->d_sptrA, s->d_wordsA, zpad);
  HIPCK(hipGetLastError());
  // ---- segment B: slices of <= 64 rows of one block, chunk-major
  const SectorTables& T = s->T;
  const int64_t nblk = (int64_t)T.blk_off.size() - 1;
  int64_t maxlen = 0;
  for (int64_t b = 0; b < nblk; b++) maxlen = std::max(maxlen, T.blk_off[b + 1] - T.blk_off[b]);
  std::vector<SplitSlice> sl;
  const int64_t R = kSplitRows;
  const int64_t nchunk = (maxlen + R - 1) / R;
  std::vector<int32_t> sid(nchunk * nblk, -1);  // slice of (chunk, block)
  for (int64_t c = 0; c * R < maxlen; c++)
    for (int64_t b = 0; b < nblk; b++) {
      const int64_t len = T.blk_off[b + 1] - T.blk_off[b];
      if (c * R >= len) continue;
      sid[c * nblk + b] = (int32_t)sl.size();
      SplitSlice q{};
      q.row0 = (int32_t)(T.blk_off[b] + c * R);
      q.nfl = (int32_t)std::min<int64_t>(R, len - c * R);
      sl.push_back(q);
    }
  const int64_t nsl = (int64_t)sl.size();
  CK(dalloc_t(s, &s->d_bsl, std::max<int64_t>(nsl, 1)));
  CK(dcopy(s, s->d_bsl, sl.data(), nsl * sizeof(SplitSlice), hipMemcpyHostToDevice));
  const int gb = (int)std::min<int64_t>((nsl + 1) / 2, 65536);
  hipLaunchKernelGGL(k_split_b<false>, dim3(gb), dim3(kSplitBuildBlock), 0, s->stream, s->d_sptr, s->d_words, s->d_cnt,
                     s->d_map, nsp, s->d_bsl, nsl, (int2*)nullptr, (uint32_t*)nullptr, zpad);
  HIPCK(hipGetLastError());
  CK(dcopy(s, sl.data(), s->d_bsl, nsl * sizeof(SplitSlice), hipMemcpyDeviceToHost));
  int64_t uo = 0, lo = 0, nfar_u = 0;
  int numax = 0;
  for (const SplitSlice& q : sl) numax = std::max(numax, q.nu);
  // U batch of segment B: 7 where no slice has more (Nlevels=28 half
  // filling: every row has 7 down-spin hops; a batch of 8 gathers the pad)
  const int uch = numax == 7 ? 7 : kSplitChunk;
  s->split_uch = uch;
  for (SplitSlice& q : sl) {
    nfar_u += (int64_t)q.nu * split_n(q);
    q.nu = (q.nu + uch - 1) / uch * uch;  // padded with {0, zero value}
    q.wl = (q.wl + kSplitLChunk - 1) / kSplitLChunk * kSplitLChunk;
    q.uoff = uo;
    q.loff = lo;
    uo += q.nu;
    lo += kSplitRows * (int64_t)q.wl;
  }
  // Default policy: the two-segment form only where (nearly) every
  // cross-block element is uniform over its slice (normal-mode sectors
  // without Jx/Jp: the down-spin hops).  With per-row L words (spin flips,
  // Jx/Jp) it is slower: N28 with Jx/Jp (95.7 % uniform) 0.308 vs 0.283 ms
  // one-pass, nonSU2 N26 (39 %) 0.493 vs 0.380 (profiles/r5).
  if (!(s->flags & ED_SPLIT_ON) && (double)nfar_u < 0.99 * (double)nfar) {
    scratch_free();
    dfree(s, (void**)&s->d_bsl, nsl * sizeof(SplitSlice));
    dfree(s, (void**)&s->d_wordsA, std::max<int64_t>(slotsA, 1) * sizeof(uint32_t));
    dfree(s, (void**)&s->d_sptrA, (ns + 1) * sizeof(int64_t));
    s->paddedA = 0;
    return ED_OK;
  }
  CK(dcopy(s, s->d_bsl, sl.data(), nsl * sizeof(SplitSlice), hipMemcpyHostToDevice));
  // (+ one chunk: a two-slice batch may read a whole chunk at a slice with no U entries)
  CK(dalloc_t(s, &s->d_ul, uo + kSplitChunk));
  HIPCK(hipMemsetAsync(s->d_ul, 0, (uo + kSplitChunk) * sizeof(int2), s->stream));
  CK(dalloc_t(s, &s->d_lw, std::max<int64_t>(lo, 1)));
  hipLaunchKernelGGL(k_split_b<true>, dim3(gb), dim3(kSplitBuildBlock), 0, s->stream, s->d_sptr, s->d_words, s->d_cnt,
                     s->d_map, nsp, s->d_bsl, nsl, s->d_ul, s->d_lw, zpad);
  HIPCK(hipGetLastError());
  // work lists in half-chunk-major order (k_spmv_sb)
  std::vector<int2> itR;
  std::vector<int> gl;
  int pend = -1;
  for (int64_t c64 = 0; c64 < 2 * nchunk; c64++)
    for (int64_t b = 0; b < nblk; b++) {
      const int32_t id = sid[(c64 / 2) * nblk + b];
      if (id < 0) continue;
      const int h = (int)(c64 & 1);
      const SplitSlice& q = sl[id];
      if (64 * h >= split_n(q)) continue;
      const int e = 2 * id + h;
      if (!(split_flags(q) & kSplitPair)) {
        if (h == 0) gl.push_back(id);
        continue;
      }
      if (pend < 0) {
        pend = e;
      } else if (sl[pend >> 1].nu == q.nu && sl[pend >> 1].wl == q.wl) {
        itR.push_back(make_int2(pend, e));
        pend = -1;
      } else {
        itR.push_back(make_int2(pend, -1));
        pend = e;
      }
    }
  if (pend >= 0) itR.push_back(make_int2(pend, -1));
  // per-XCD ranges: eight equal contiguous parts of each list
  std::vector<int> xo(27);
  for (int x = 0; x <= 8; x++) {
    xo[x] = (int)((int64_t)itR.size() * x / 8);
    xo[9 + x] = (int)((int64_t)gl.size() * x / 8);
  }
  if (itR.empty()) itR.push_back(make_int2(0, -1));
  if (gl.empty()) gl.push_back(0);
  CK(upload(s, &s->d_itR, itR));
  // bytes one launch reads besides the U / L entries: segment A's slice
  // pointers and the work list of the real (or complex) form
  s->split_meta = (ns + 1) * 8;
  s->split_listR = (int64_t)itR.size() * 8 + (int64_t)gl.size() * 4 + nsl * (int64_t)sizeof(SplitSlice);
  CK(upload(s, &s->d_glist, gl));
  CK(upload(s, &s->d_xoff, xo));
  scratch_free();
  s->nbsl = (int)nsl;
  s->nul = uo;
  s->nlw = lo;
  s->nfar_u = nfar_u;
  s->nfar = nfar;
  s->split = true;
  return ED_OK;
}

// ---------------------------------------------- fused one-pass stored H
// (ed_fused.hpp).  Built where the two-segment form is considered (whole
// packed sectors beyond the Infinity Cache) and on request (ED_FUSED_ON).
static int build_fused(ed_sector* s) {
  const int hw = s->hc ? 2 : 1;
  const int nsp = s->Mh.ns;
  // the dictionary's zero (padding slots); appended when absent
  std::vector<double> dict(256 * hw);
  CK(dcopy(s, dict.data(), s->d_pdict, dict.size() * 8, hipMemcpyDeviceToHost));
  int z = -1;
  for (int k = 0; k < s->npdict && z < 0; k++) {
    bool zero = true;
    for (int h = 0; h < hw; h++) zero = zero && dict[k * hw + h] == 0.0 && !std::signbit(dict[k * hw + h]);
    if (zero) z = k;
  }
  if (z < 0) {
    if (s->npdict >= 256) return ED_OK;  // no room for a zero: the one-pass kernel serves
    z = s->npdict++;
    HIPCK(hipMemsetAsync((double*)s->d_pdict + (size_t)z * hw, 0, 8 * hw, s->stream));
  }
  const uint32_t zpad = (uint32_t)z << kPackShift;
  // units: <= 64 consecutive rows of one idw block, row order
  const SectorTables& T = s->T;
  const int64_t nblk = (int64_t)T.blk_off.size() - 1;
  std::vector<FuUnit> un;
  for (int64_t b = 0; b < nblk; b++)
    for (int64_t r = T.blk_off[b]; r < T.blk_off[b + 1]; r += 64) {
      FuUnit u{};
      u.row0 = (int32_t)r;
      u.n = (int32_t)std::min<int64_t>(64, T.blk_off[b + 1] - r);
      un.push_back(u);
    }
  const int64_t nu = (int64_t)un.size();
  if (nu == 0) return ED_OK;
  CK(upload(s, &s->d_fu, un));
  int* farmax;  // [0]: largest cross-block count of a row; [2..3]: cross-block total
  HIPCK(hipMallocAsync((void**)&farmax, 16, s->stream));
  HIPCK(hipMemsetAsync(farmax, 0, 16, s->stream));
  const int gb = (int)std::min<int64_t>((nu + 3) / 4, 65536);
  hipLaunchKernelGGL(k_fu_build<false>, dim3(gb), dim3(kFuBuildBlock), 0, s->stream, s->d_sptr, s->d_words, s->d_cnt,
                     s->d_map, nsp, s->d_fu, nu, (uint32_t*)nullptr, (int2*)nullptr, (uint32_t*)nullptr, zpad, farmax,
                     (unsigned long long*)(farmax + 2));
  HIPCK(hipGetLastError());
  int hfar[4] = {0, 0, 0, 0};
  HIPCK(hipMemcpyAsync(hfar, farmax, 16, hipMemcpyDeviceToHost, s->stream));
  CK(dcopy(s, un.data(), s->d_fu, nu * sizeof(FuUnit), hipMemcpyDeviceToHost));
  (void)hipFreeAsync(farmax, s->stream);
  unsigned long long far_all = 0;
  memcpy(&far_all, hfar + 2, 8);
  if (hfar[0] > kFuFarMax) {  // rows with more cross-block elements than the build stages
    dfree(s, (void**)&s->d_fu, nu * sizeof(FuUnit));
    return ED_OK;
  }
  int numax = 0;
  for (const FuUnit& u : un) numax = std::max(numax, u.nu);
  // U batch: 7 where no unit has more (Nlevels=28 half filling: 7 down hops)
  const int uch = numax == 7 ? 7 : kFuUChunk;
  int64_t ao = 0, uo = 0, lo = 0, far_u = 0;
  int wmax = 0, wmin = 1 << 30;
  for (FuUnit& u : un) {
    far_u += (int64_t)u.nu * u.n;
    wmax = std::max(wmax, u.wa);
    wmin = std::min(wmin, u.wa);
    u.nu = (u.nu + uch - 1) / uch * uch;
    u.wl = (u.wl + kFuLChunk - 1) / kFuLChunk * kFuLChunk;
    u.aoff = ao;
    u.uoff = uo;
    u.loff = lo;
    ao += 64 * (int64_t)u.wa;
    uo += u.nu;
    lo += 64 * (int64_t)u.wl;
  }
  // Default policy: only where (nearly) every cross-block element is
  // unit-uniform.  nonSU2 spin flips stay per-lane L words: N26 (41 % in U)
  // 0.394 vs 0.380 ms one-pass for real vectors, 0.556 vs 0.530 complex H
  // (gpurun_out r6c); N28 with Jx/Jp (95.7 %) gains (0.242 vs 0.275).
  if (!(s->flags & ED_FUSED_ON) && (double)far_u < 0.9 * (double)far_all) {
    dfree(s, (void**)&s->d_fu, nu * sizeof(FuUnit));
    return ED_OK;
  }
  CK(dcopy(s, s->d_fu, un.data(), nu * sizeof(FuUnit), hipMemcpyHostToDevice));
  CK(dalloc_t(s, &s->d_fa, std::max<int64_t>(ao, 1)));
  CK(dalloc_t(s, &s->d_ful, uo + kFuUChunk));
  HIPCK(hipMemsetAsync(s->d_ful, 0, (uo + kFuUChunk) * sizeof(int2), s->stream));
  CK(dalloc_t(s, &s->d_flw, std::max<int64_t>(lo, 1)));
  hipLaunchKernelGGL(k_fu_build<true>, dim3(gb), dim3(kFuBuildBlock), 0, s->stream, s->d_sptr, s->d_words, s->d_cnt,
                     s->d_map, nsp, s->d_fu, nu, s->d_fa, s->d_ful, s->d_flw, zpad, (int*)nullptr,
                     (unsigned long long*)nullptr);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(s->stream));
  s->nfu = nu;
  s->fu_far = (int64_t)far_all;
  s->fu_na = ao;
  s->fu_nu = uo;
  s->fu_nl = lo;
  s->fu_far_u = far_u;
  s->fu_wa_max = wmax;
  s->fu_wa_min = wmin;
  s->fu_uch = uch;
  s->fused = true;
  return ED_OK;
}

int build_stored(ed_sector* s) {
  const int64_t dim = s->nrows, ns = s->nslice;  // rows held by this sector object
  const uint32_t* map = s->d_map + s->row0;
  uint16_t* cnt;
  int32_t* width;
  int64_t* bsum;
  int64_t* total;
  CK(dalloc_t(s, &cnt, dim));
  s->d_cnt = cnt;
  // width/bsum/total are scratch, freed right after the build
  HIPCK(hipMallocAsync((void**)&width, ns * sizeof(int32_t), s->stream));
  int64_t nb = (ns + 1023) / 1024;
  HIPCK(hipMallocAsync((void**)&bsum, std::max<int64_t>(nb, 1) * sizeof(int64_t), s->stream));
  HIPCK(hipMallocAsync((void**)&total, sizeof(int64_t), s->stream));
  CK(dalloc_t(s, &s->d_sptr, ns + 1));
  hipLaunchKernelGGL(k_count, dim3(grid_for(ns * 64)), dim3(kBlock), 0, s->stream, s->Md, map,
                     dim, ns, cnt, width);
  HIPCK(hipGetLastError());
  hipLaunchKernelGGL(k_scan_blocks, dim3((unsigned)nb), dim3(1024), 0, s->stream, width, ns,
                     s->d_sptr, bsum);
  hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(64), 0, s->stream, bsum, nb, total);
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(1024), 0, s->stream, s->d_sptr, ns,
                     bsum, total);
  HIPCK(hipGetLastError());
  int64_t slots = 0;
  HIPCK(hipMemcpyAsync(&slots, total, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  (void)hipFreeAsync(width, s->stream);
  (void)hipFreeAsync(bsum, s->stream);
  (void)hipFreeAsync(total, s->stream);
  s->padded = slots;
  const size_t hv = s->hc ? 16 : 8;
  CK(dalloc(s, &s->d_diag, dim * hv));
  CK(dalloc_t(s, &s->d_cols, slots));
  CK(dalloc(s, &s->d_vals, slots * hv));
  DevIndex idx{s->d_off, s->d_rank, s->T.ns, s->T.nst - 1};
  if (s->hc)
    hipLaunchKernelGGL(k_fill<true>, dim3(grid_for(dim)), dim3(kBlock), 0, s->stream, s->Md,
                       map, dim, idx, s->d_sptr, (double2*)s->d_diag, s->d_cols,
                       (double2*)s->d_vals);
  else
    hipLaunchKernelGGL(k_fill<false>, dim3(grid_for(dim)), dim3(kBlock), 0, s->stream, s->Md,
                       map, dim, idx, s->d_sptr, (double*)s->d_diag, s->d_cols,
                       (double*)s->d_vals);
  HIPCK(hipGetLastError());
  // nnz = dim (diagonal) + sum(cnt), reduced on the device (no D2H of the counts)
  unsigned long long* dn;
  HIPCK(hipMallocAsync((void**)&dn, sizeof(unsigned long long), s->stream));
  HIPCK(hipMemsetAsync(dn, 0, sizeof(unsigned long long), s->stream));
  hipLaunchKernelGGL(k_sum_u16, dim3(grid_once(dim)), dim3(kBlock), 0, s->stream, cnt, dim, dn);
  HIPCK(hipGetLastError());
  unsigned long long hn = 0;
  HIPCK(hipMemcpyAsync(&hn, dn, sizeof(hn), hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  (void)hipFreeAsync(dn, s->stream);
  s->nnz = dim + (int64_t)hn;
  if (s->dim <= (int64_t)kPackColMask + 1 && !(s->flags & ED_NO_PACK)) CK(build_pack(s));
  if (s->d_words && !s->hc && s->row0 == 0 && s->nrows == s->dim &&
      (stored_mbytes(s) > kSplitMinBytes || (s->flags & ED_SPLIT_ON)) && !(s->flags & ED_NO_SPLIT))
    CK(build_split(s));
  if (s->d_words && s->row0 == 0 && s->nrows == s->dim &&
      (stored_mbytes(s) > kSplitMinBytes || (s->flags & ED_FUSED_ON)) && !(s->flags & ED_NO_FUSED))
    CK(build_fused(s));
  return ED_OK;
}

// ------------------------------------------------ matrix-free (generic)
// Host side of k_direct: the candidates of gen_row (direct_candidates), the
// op list of every idw block (down-only terms resolved per block into a row
// offset and a signed value, terms that cannot act in the block dropped,
// padded to kDirGroup), the 64-row chunks of the held rows and the 16-bit
// rank / by-class pattern tables.
struct RecAcc {
  std::vector<uint32_t> k;
  std::vector<double> re, im;
  double dr = 0.0, di = 0.0;
  void diag(double r, double i) { dr = r; di = i; }
  void off(uint32_t t, double r, double i) {
    k.push_back(t);
    re.push_back(r);
    im.push_back(i);
  }
};
static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// The candidates must reproduce gen_row element by element (target, value
// bits, order): checked on sample states of the sector before any launch.
static int direct_candidates_check(const ed_sector* s, const std::vector<DirCand>& cands) {
  const SectorTables& T = s->T;
  const int64_t nb = (int64_t)T.blk_idw.size();
  const int64_t step = std::max<int64_t>(1, s->dim / 4096);
  for (int64_t i = 0; i < s->dim; i += step) {
    const int64_t b = std::upper_bound(T.blk_off.begin(), T.blk_off.begin() + nb + 1, i) - T.blk_off.begin() - 1;
    const uint32_t idw = T.blk_idw[b];
    const uint32_t m = T.by_cls[T.cls_start[T.need_cls[idw]] + (i - T.blk_off[b])] | (idw << T.ns);
    RecAcc ref;
    gen_row(s->Mh, m, ref);
    size_t q = 0;
    for (const DirCand& c : cands) {
      uint32_t k;
      double sg;
      if (!cand_apply(c, m, &k, &sg)) continue;
      const double re = c.re * sg, im = c.im_signed ? c.im * sg : c.im;
      if (q >= ref.k.size() || ref.k[q] != k || !same_bits(ref.re[q], re) || !same_bits(ref.im[q], im))
        return fail(ED_ERR_STATE, "direct candidates differ from gen_row (row " + std::to_string(i) + ")");
      q++;
    }
    if (q != ref.k.size()) return fail(ED_ERR_STATE, "direct candidates miss elements of gen_row");
  }
  return ED_OK;
}

// Merge LANE op b into a (previous op of the same block) when they are the two
// directions of one hop: same two flip bits (up levels), same value and
// target block, conditions equal except on the flip bits where they read
// (1,0) and (0,1), and a Jordan-Wigner parity that agrees once the flip bits'
// part of popc(m & smask) is folded into the constant.
static bool dir_merge(DirOp& a, const DirOp& b, uint32_t nst) {
  if (!(a.kind & kDirLane) || (a.kind & kDirXor) || !(b.kind & kDirLane)) return false;
  const uint32_t fl = a.flip;
  if (fl != b.flip || __builtin_popcount(fl) != 2 || (fl & ~(nst - 1)) != 0) return false;
  if (a.delta != b.delta || !same_bits(a.re, b.re) || !same_bits(a.im, b.im) ||
      (a.kind & kDirImSigned) != (b.kind & kDirImSigned) || a.smask != b.smask)
    return false;
  if (a.req_mask != b.req_mask || (a.req_mask & fl) != fl) return false;
  if ((a.req_mask & ~fl & (nst - 1)) != 0) return false;  // (the kernel's single condition form)
  if ((a.req_val & ~fl) != (b.req_val & ~fl)) return false;
  const uint32_t va = a.req_val & fl, vb = b.req_val & fl;
  if (__builtin_popcount(va) != 1 || (va ^ vb) != fl) return false;
  const int pa = (__builtin_popcount(va & a.smask) + ((a.kind & kDirC0) ? 1 : 0)) & 1;
  const int pb = (__builtin_popcount(vb & b.smask) + ((b.kind & kDirC0) ? 1 : 0)) & 1;
  if (pa != pb) return false;
  a.req_mask &= ~fl;
  a.req_val &= ~fl;
  a.smask &= ~fl;
  a.xm = fl;
  a.kind = (a.kind & ~kDirC0) | (pa ? kDirC0 : 0) | kDirXor;
  return true;
}

// Op q of a block (down pattern idw, first row own0) folded into slot j of
// a kernel group: conditions, flip and string mask restricted to the up
// pattern; the sign part fixed by the block's down bits and the string's
// constant multiplied into the value (a sign flip: the same bits as the
// reference's products by +-1).  Pads become UNI ops of value 0 on the
// row's own entry.
static void dir_fold(const DirOp& o, uint32_t idw, int ns, uint32_t nst, int64_t own0, DirGroup& G, int j) {
  const uint32_t um = nst - 1, mdw = idw << ns;
  G.cmask[j] = G.cval[j] = G.flipu[j] = G.smasku[j] = G.xm[j] = G.xv[j] = 0;
  if (o.kind & kDirPad) {
    G.delta[j] = (int32_t)own0;
    G.re[j] = G.im[j] = 0.0;
    return;
  }
  const bool ims = (o.kind & kDirImSigned) != 0;
  int neg;
  if (o.kind & kDirLane) {
    G.lanes |= 1u << j;
    // one condition form: popc((u ^ cval) & cmask) == xv — the op's bit
    // conditions (xv = 0), or a merged hop pair's "exactly one of the two
    // bits" (xv = 1; dir_merge leaves such an op no other up-bit condition)
    G.xm[j] = o.xm & um;
    if (o.kind & kDirXor) {
      G.cmask[j] = o.xm & um;
      G.cval[j] = 0;
      G.xv[j] = 1;
    } else {
      G.cmask[j] = o.req_mask & um;
      G.cval[j] = o.req_val & um;
      G.xv[j] = 0;
    }
    G.flipu[j] = o.flip & um;
    G.smasku[j] = o.smask & um;
    if (ims) G.imsig |= 1u << j;
    neg = (__builtin_popcount(mdw & o.smask) + ((o.kind & kDirC0) ? 1 : 0)) & 1;
  } else {
    neg = (o.kind & kDirC0) ? 1 : 0;  // the block's whole sign (build_direct)
  }
  G.delta[j] = o.delta;
  G.re[j] = neg ? -o.re : o.re;
  G.im[j] = (neg && ims) ? -o.im : o.im;
}

// The kernel's view of op j of a group (host restatement of dir_group):
// fires?, target row, value.
static bool dir_eval(const DirGroup& G, int j, uint32_t up, const std::vector<uint32_t>& rank, int64_t* tgt,
                     double* re, double* im) {
  if (!((G.lanes >> j) & 1u)) {
    *tgt = G.delta[j] + (int64_t)rank[up];
    *re = G.re[j];
    *im = G.im[j];
    return true;
  }
  const bool f = (uint32_t)__builtin_popcount((up ^ G.cval[j]) & G.cmask[j]) == G.xv[j];
  if (!f) return false;
  const bool neg = (__builtin_popcount(up & G.smasku[j]) & 1) != 0;
  *tgt = G.delta[j] + (int64_t)rank[up ^ G.flipu[j]];
  *re = neg ? -G.re[j] : G.re[j];
  *im = (neg && ((G.imsig >> j) & 1u)) ? -G.im[j] : G.im[j];
  return true;
}

// The final kernel groups against gen_row on sample rows: targets (through
// the sector's index), value bits and order (pads: zero products only).
static int direct_ops_check(const ed_sector* s, const std::vector<DirGroup>& groups, const std::vector<uint8_t>& pad,
                            const std::vector<DirChunk>& chunks) {
  const SectorTables& T = s->T;
  const size_t step = std::max<size_t>(1, chunks.size() / 512);
  for (size_t ci = 0; ci < chunks.size(); ci += step) {
    const DirChunk& ch = chunks[ci];
    for (int l = 0; l < ch.n; l += std::max(1, ch.n / 8)) {
      const int64_t row = ch.row + l;
      const uint32_t up = T.by_cls[ch.pat0 + l];
      const uint32_t m = up | (ch.idw << T.ns);
      RecAcc ref;
      gen_row(s->Mh, m, ref);
      size_t q = 0;
      for (int k = ch.op0; k < ch.op0 + ch.nop; k++) {
        const DirGroup& G = groups[k / kDirGroup];
        const int j = k % kDirGroup;
        int64_t tg;
        double re, im;
        if (!dir_eval(G, j, up, T.rank, &tg, &re, &im)) continue;
        if (pad[k]) {
          if (re != 0.0 || im != 0.0 || tg != row) return fail(ED_ERR_STATE, "direct: pad op is not a zero product");
          continue;
        }
        if (q >= ref.k.size() || table_index(T, ref.k[q]) != tg || !same_bits(ref.re[q], re) ||
            !same_bits(ref.im[q], im))
          return fail(ED_ERR_STATE, "direct op lists differ from gen_row (row " + std::to_string(row) + ")");
        q++;
      }
      if (q != ref.k.size()) return fail(ED_ERR_STATE, "direct op lists miss elements of gen_row");
    }
  }
  return ED_OK;
}

int build_direct(ed_sector* s) {
  const SectorTables& T = s->T;
  const int ns = T.ns;
  const uint32_t nst = T.nst;
  std::vector<DirCand> cands;
  direct_candidates(s->Mh, cands);
  CK(direct_candidates_check(s, cands));
  std::vector<DirOp> ops;
  std::vector<DirChunk> chunks, chunks2;  // 64- and 128-row chunks
  std::vector<std::pair<uint32_t, int64_t>> opblk;  // per op: (idw, first row) of its block
  const int64_t r0 = s->row0, r1 = s->row0 + s->nrows;
  for (size_t b = 0; b + 1 < T.blk_off.size(); b++) {
    const int64_t lo = std::max<int64_t>(T.blk_off[b], r0), hi = std::min<int64_t>(T.blk_off[b + 1], r1);
    if (lo >= hi) continue;
    const uint32_t idw = T.blk_idw[b];
    const uint32_t mdw = idw << ns;
    const int32_t op0 = (int32_t)ops.size();
    for (const DirCand& c : cands) {
      const uint32_t dmask = ~(nst - 1);  // down levels
      if ((mdw & c.req_mask & dmask) != (c.req_val & dmask)) continue;  // cannot act in this block
      const uint32_t idw2 = idw ^ (c.flip >> ns);
      const int32_t off2 = T.off[idw2];
      const bool uni = ((c.req_mask | c.flip | c.smask) & (nst - 1)) == 0;
      DirOp o{};
      if (uni) {
        // no up bits: always fires in this block, the lane's own rank in the
        // target block, the block's Jordan-Wigner sign in c0
        if (off2 < 0) return fail(ED_ERR_STATE, "direct: a down-level term leaves the sector");
        const int neg = (__builtin_popcount(mdw & c.smask) + c.c0) & 1;
        o.delta = off2;
        o.kind = (neg ? kDirC0 : 0) | (c.im_signed ? kDirImSigned : 0);
        o.re = c.re;
        o.im = c.im;
      } else {
        if (off2 < 0) continue;  // no up pattern can reach an empty block
        o.req_mask = c.req_mask;
        o.req_val = c.req_val;
        o.flip = c.flip;
        o.smask = c.smask;
        o.delta = off2;
        o.kind = kDirLane | (c.c0 ? kDirC0 : 0) | (c.im_signed ? kDirImSigned : 0);
        o.re = c.re;
        o.im = c.im;
      }
      // the two directions of a hop (c+_a c_b then c+_b c_a, adjacent in
      // gen_row order, exclusive conditions): one op firing on "exactly one
      // of the two flip bits set" (halves the per-lane op evaluations)
      if (!uni && (int32_t)ops.size() > op0 && dir_merge(ops.back(), o, nst)) continue;
      ops.push_back(o);
    }
    while ((ops.size() - op0) % kDirGroup) {
      DirOp o{};
      o.req_val = 1;  // (m & 0) != 1: never fires
      o.kind = kDirPad;
      ops.push_back(o);
    }
    const int32_t nop = (int32_t)ops.size() - op0;
    opblk.resize(ops.size(), std::make_pair(idw, T.blk_off[b]));
    const int64_t cls0 = T.cls_start[T.need_cls[idw]];
    for (int rr = 0; rr < 2; rr++)
      for (int64_t r = lo; r < hi; r += 64 << rr) {
        DirChunk ch{};
        ch.row = (int32_t)r;
        ch.idw = idw;
        ch.pat0 = (int32_t)(cls0 + (r - T.blk_off[b]));
        ch.n = (int32_t)std::min<int64_t>(64 << rr, hi - r);
        ch.op0 = op0;
        ch.nop = nop;
        (rr ? chunks2 : chunks).push_back(ch);
      }
  }
  std::vector<DirGroup> groups(std::max<size_t>(ops.size() / kDirGroup, 1));  // (valid pointer)
  std::vector<uint8_t> pad(ops.size(), 0);
  for (size_t q = 0; q < ops.size(); q++) {
    dir_fold(ops[q], opblk[q].first, ns, nst, opblk[q].second, groups[q / kDirGroup], (int)(q % kDirGroup));
    pad[q] = (ops[q].kind & kDirPad) ? 1 : 0;
  }
  CK(direct_ops_check(s, groups, pad, chunks));
  std::vector<uint16_t> rk(std::max<uint32_t>(nst, 8), 0), pt(std::max<uint32_t>(nst, 8), 0);
  for (uint32_t x = 0; x < nst; x++) {
    rk[x] = (uint16_t)T.rank[x];
    pt[x] = (uint16_t)T.by_cls[x];
  }
  s->ndchunk = (int)chunks.size();
  s->ndchunk2 = (int)chunks2.size();
  if (chunks.empty()) chunks.resize(1);
  if (chunks2.empty()) chunks2.resize(1);
  CK(upload(s, &s->d_dchunk, chunks));
  CK(upload(s, &s->d_dchunk2, chunks2));

  CK(upload(s, &s->d_dops, groups));
  CK(upload(s, &s->d_rank16, rk));
  CK(upload(s, &s->d_pat16, pt));
  // the rows' diagonal, once (k_direct reads it instead of running gen_diag)
  CK(dalloc(s, &s->d_ddiag, (size_t)std::max<int64_t>(s->nrows, 1) * (s->hc ? 16 : 8)));
  if (s->nrows > 0) {
    if (s->hc)
      hipLaunchKernelGGL(k_gen_diag<true>, dim3(grid_for(s->nrows)), dim3(kBlock), 0, s->stream, s->Md,
                         s->d_map + s->row0, s->nrows, (double2*)s->d_ddiag);
    else
      hipLaunchKernelGGL(k_gen_diag<false>, dim3(grid_for(s->nrows)), dim3(kBlock), 0, s->stream, s->Md,
                         s->d_map + s->row0, s->nrows, (double*)s->d_ddiag);
    HIPCK(hipGetLastError());
  }
  // both tables in LDS up to Ns = 15 (128 KB); at Ns = 16 the rank table
  // alone (128 KB), the row's own pattern then read from H%map
  s->dir_patlds = 4 * (int64_t)rk.size() <= 128 * 1024;
  s->dir_lds = (int)((s->dir_patlds ? 4 : 2) * rk.size());
  // 16 chunks per workgroup and step; at most 2 workgroups per CU: the
  // fixed grid also sizes the per-block partials of fused epilogues
  const int g = (int)std::min<int64_t>((s->ndchunk + 15) / 16, 512);
  s->dir_grid = g >= 8 ? (g & ~7) : std::max(g, 1);
  return ED_OK;
}

// the k_direct tables on first use of path 1 (build_direct), ordered before
// the caller's stream by a sync of the sector's stream
int ensure_direct(ed_sector* s, int path, hipStream_t caller) {
  if (path != 1 || s->nrows == 0) return ED_OK;
  // one builder per sector (two threads' first path-1 H·v would race on the
  // tables); a stream being graph-captured cannot take the build's syncs
  std::lock_guard<std::mutex> lk(s->build_mu);
  if (s->d_dchunk) return ED_OK;
  if (caller) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(caller, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(ED_ERR_STATE, "first generic matrix-free H·v inside a graph capture: run one outside first");
  }
  if (!(s->flags & ED_DIRECT)) return fail(ED_ERR_ARG, "generic matrix-free path needs ED_DIRECT");
  CK(build_direct(s));
  HIPCK(hipStreamSynchronize(s->stream));
  return ED_OK;
}

// ---------------------------------------------------- Kronecker (normal)
struct HopAcc {
  std::vector<uint32_t> tgt;
  std::vector<double> re, im;
  void diag(double, double) {}
  void off(uint32_t k, double r, double i) {
    tgt.push_back(k);
    re.push_back(r);
    im.push_back(i);
  }
};

// Separable one-body diagonal of one spin species (Himp diag + Hbath diag).
static void spin_diag(const EdModel& M, int sp, uint32_t x, double* re, double* im) {
  const int ss = sp == 0 ? 0 : M.S;
  double r = 0.0, i = 0.0;
  for (int o = 0; o < M.norb; o++) {
    double n = (double)bit(x, o);
    r = r + M.hloc_re[ss][ss][o][o] * n;
    i = i + M.hloc_im[ss][ss][o][o] * n;
    r = r - M.xmu * n;
  }
  if (M.bath != ED_BATH_REPLICA) {
    for (int o = 0; o < M.ne; o++)
      for (int k = 0; k < M.nbath; k++) r = r + M.e[ss][o][k] * (double)bit(x, M.stride[o][k]);
  } else {
    for (int k = 0; k < M.nbath; k++)
      for (int o = 0; o < M.norb; o++) {
        double n = (double)bit(x, M.stride[o][k]);
        r = r + M.hb_re[ss][ss][o][o][k] * n;
        i = i + M.hb_im[ss][ss][o][o][k] * n;
      }
  }
  *re = r;
  *im = i;
}

// Two-pass Kronecker tables (k_kron_up): the up-hop ELL slots as 32-bit words
// {column:16 | index:8} over a dictionary of the distinct values (bit
// patterns: exact).  Only for large sectors (dim >= 2^19; the small ones run
// in the persistent kernels) whose up rows fit the register and LDS budget.
// crossover with the one-pass k_kron on configs[3] sectors: dim 392,040 0.0108
// vs 0.0111 ms, 627,264 0.0223 vs 0.0155 ms (tools/kron2_threshold.py)
static constexpr int64_t kKron2MinDim = (int64_t)1 << 19;
// Slot bound of a template instantiation (8, 12 or 16 hops per row).
static int kron_slot_bound(int deg) { return deg <= 8 ? 8 : deg <= 12 ? 12 : 16; }

static int build_kron_words(ed_sector* s, int sp, const std::vector<int32_t>& cols,
                            const std::vector<double>& vals, int64_t nr, int deg,
                            const std::vector<uint8_t>& nhop) {
  KronHost& K = s->K;
  if (sp == 0) {
    K.two = false;
    if (s->flags & ED_KRON2_OFF) return ED_OK;
    if (s->dim < kKron2MinDim && !(s->flags & ED_KRON2_ON)) return ED_OK;
    if (nr > 8192 || deg > 16 || s->dim >= ((int64_t)1 << 31)) return ED_OK;  // 32-bit element offsets
    if (K.nimp * K.nimp > kKronUimpMax) return ED_OK;                          // U table in LDS
    int cpt = 1;
    while (cpt * kKronUpBlock < nr) cpt *= 2;
    K.cpt = cpt;
    K.degU = kron_slot_bound(deg);
    // the thread's up-hop words live in VGPRs: cpt x DEG of them (4 x 16 at
    // DimUp > 2048 spilled to scratch: 3x slower pass U)
    if (cpt * K.degU > (K.degU == 8 ? 64 : 48)) return ED_OK;
    K.two = true;
  } else {
    if (!K.two) return ED_OK;
    K.two = false;
    if (nr > 65535 || deg > 16) return ED_OK;
    K.degD = kron_slot_bound(deg);
  }
  const int hw = s->hc ? 2 : 1;
  std::map<std::pair<uint64_t, uint64_t>, uint32_t> idx;
  std::vector<double> dict;
  std::vector<uint32_t> words((size_t)deg * nr);
  for (size_t q = 0; q < words.size(); q++) {
    uint64_t x0 = 0, x1 = 0;
    memcpy(&x0, &vals[hw * q], 8);
    if (hw == 2) memcpy(&x1, &vals[2 * q + 1], 8);
    auto it = idx.find({x0, x1});
    uint32_t id;
    if (it == idx.end()) {
      id = (uint32_t)idx.size();
      if (id >= (uint32_t)kKronDictMax) {  // too many distinct values: one-pass k_kron
        K.two = false;
        return ED_OK;
      }
      idx[{x0, x1}] = id;
      for (int c = 0; c < hw; c++) dict.push_back(vals[hw * q + c]);
    } else {
      id = it->second;
    }
    words[q] = (uint32_t)cols[q] | (id << 16);
  }
  void*& dp = sp == 0 ? K.updict : K.dwdict;
  if (sp == 0) {
    CK(upload(s, &K.upw, words));
  } else {
    // pass D layout: [row][DEG slot] target rows (the kernel scales them by
    // its row length) and value indices
    // Slot 0's word also carries the row's hop count in bits 24..31: the
    // padding slots (own row, zero value) trail the hops, and pass D skips
    // them with a wave-uniform branch (Norb=2 rows hold 0..12 hops in 12 slots)
    std::vector<uint32_t> off((size_t)nr * K.degD, 0u);
    std::vector<uint8_t> ix((size_t)nr * K.degD, 0);
    for (int64_t r = 0; r < nr; r++) {
      for (int k = 0; k < deg; k++) {
        const uint32_t wd = words[(size_t)k * nr + r];
        off[(size_t)r * K.degD + k] = wd & 0xffffu;
        ix[(size_t)r * K.degD + k] = (uint8_t)(wd >> 16);
      }
      off[(size_t)r * K.degD] |= (uint32_t)nhop[r] << 24;
    }
    CK(upload(s, &K.dwo, off));
    CK(upload(s, &K.dwi, ix));
  }
  CK(dalloc(s, &dp, dict.size() * 8));
  CK(dcopy(s, dp, dict.data(), dict.size() * 8, hipMemcpyHostToDevice));
  (sp == 0 ? K.nupdict : K.ndwdict) = (int)(dict.size() / hw);
  K.two = true;
  return ED_OK;
}

int build_kron(ed_sector* s) {
  const SectorTables& T = s->T;
  const EdModel& M = s->Mh;
  KronHost& K = s->K;
  const int nup = T.q1, ndw = T.q2;
  K.dimup = T.dimup;
  K.dimdw = T.dimdw;
  K.nimp = 1 << M.norb;
  const uint32_t mask = T.nst - 1;
  const uint32_t* ups = &T.by_cls[T.cls_start[nup]];  // normal mode: class = popcount
  const uint32_t* dws = &T.by_cls[T.cls_start[ndw]];
  const size_t hv = s->hc ? 16 : 8;
  for (int sp = 0; sp < 2; sp++) {
    const int64_t nr = sp == 0 ? K.dimup : K.dimdw;
    const uint32_t* st = sp == 0 ? ups : dws;
    std::vector<HopAcc> rows(nr);
    int deg = 0;
    for (int64_t r = 0; r < nr; r++) {
      uint32_t m = sp == 0 ? st[r] : (st[r] << M.ns);
      gen_row(M, m, rows[r]);
      deg = std::max<int>(deg, (int)rows[r].tgt.size());
    }
    std::vector<uint8_t> nhop(nr);
    for (int64_t r = 0; r < nr; r++) nhop[r] = (uint8_t)rows[r].tgt.size();
    std::vector<int32_t> cols((size_t)deg * nr);
    std::vector<double> vals((size_t)deg * nr * (s->hc ? 2 : 1), 0.0);
    for (int64_t r = 0; r < nr; r++)
      for (int k = 0; k < deg; k++) {
        size_t q = (size_t)k * nr + r;
        if (k < (int)rows[r].tgt.size()) {
          uint32_t t = rows[r].tgt[k];
          uint32_t loc = sp == 0 ? t : (t >> M.ns);
          if ((sp == 0 && (t >> M.ns) != 0) || (sp == 1 && (t & mask) != 0))
            return fail(ED_ERR_STATE, "kron: hop mixes spin species");
          cols[q] = (int32_t)T.rank[loc];
          if (s->hc) {
            vals[2 * q] = rows[r].re[k];
            vals[2 * q + 1] = rows[r].im[k];
          } else {
            vals[q] = rows[r].re[k];
          }
        } else {
          cols[q] = (int32_t)r;  // padding: own column, zero value
        }
      }
    std::vector<double> a(nr * (s->hc ? 2 : 1));
    std::vector<uint8_t> imp(nr);
    for (int64_t r = 0; r < nr; r++) {
      double re, im;
      spin_diag(M, sp, st[r], &re, &im);
      if (im != 0.0) K.diag_real = false;
      if (s->hc) {
        a[2 * r] = re;
        a[2 * r + 1] = im;
      } else {
        a[r] = re;
      }
      imp[r] = (uint8_t)(st[r] & (uint32_t)(K.nimp - 1));
    }
    int32_t* dc;
    void *dv, *da;
    uint8_t* di;
    CK(upload(s, &dc, cols));
    CK(dalloc(s, &dv, vals.size() * 8));
    CK(dcopy(s, dv, vals.data(), vals.size() * 8, hipMemcpyHostToDevice));
    CK(dalloc(s, &da, a.size() * 8));
    CK(dcopy(s, da, a.data(), a.size() * 8, hipMemcpyHostToDevice));
    CK(upload(s, &di, imp));
    CK(build_kron_words(s, sp, cols, vals, nr, deg, nhop));
    if (sp == 0) {
      K.degup = deg; K.upc = dc; K.upv = dv; K.aup = da; K.impu = di;
    } else {
      K.degdw = deg; K.dwc = dc; K.dwv = dv; K.adw = da; K.impd = di;
    }
    (void)hv;
  }
  std::vector<double> u((size_t)K.nimp * K.nimp);
  for (int x = 0; x < K.nimp; x++)
    for (int y = 0; y < K.nimp; y++) u[(size_t)x * K.nimp + y] = hint_value(M, (uint32_t)x, (uint32_t)y);
  CK(upload(s, &K.uimp, u));
  return ED_OK;
}
