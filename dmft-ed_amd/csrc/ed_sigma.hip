// ed_sigma.hip — ed_sigma_build: the self-energy, the Weiss field and the bath
// hybridisation on the device (csrc/ed_sigma.hpp, csrc/ed_sigma_host.hpp;
// DESIGN.md section 14).
#include <string.h>

#include <vector>

#include "ed_host.hpp"
#include "ed_sigma.hpp"

using namespace edg;

namespace {

template <int N>
void launch_sigma(int nblk, const SigmaBlock* dblk, const SigmaArrays& A, double beta, int lmats, double wini,
                  double wfin, int lreal, double eps, int with_g, hipStream_t st) {
  const int nt = lmats + lreal;
  hipLaunchKernelGGL(k_sigma<N>, dim3((nt + kSigBlock - 1) / kSigBlock, nblk), dim3(kSigBlock), 0, st, dblk, A, beta,
                     lmats, wini, wfin, lreal, eps, with_g);
}

// runs on the stream after the upload it follows: the staging table can go
void free_staging(void* p) { delete (std::vector<SigmaBlock>*)p; }

}  // namespace

int ed_sigma_blocks(const ed_params* p, ed_sigma_block* blocks, int32_t* nblk) {
  if (!p || !blocks || !nblk) return fail(ED_ERR_ARG, "null");
  const char* why = "";
  int n = 0;
  const int rc = sigma_blocks(*p, blocks, &n, &why);
  if (rc != ED_OK) return fail(rc, std::string("ed_sigma_blocks: ") + why);
  *nblk = n;
  return ED_OK;
}

int ed_sigma_build_blocks(int32_t nblk, const ed_sigma_block* blocks, int32_t nspin, int32_t norb, double beta,
                          int32_t lmats, double wini, double wfin, int32_t lreal, double eps, const double* gm,
                          const double* gr, const double* fm, const double* fr, double* smats, double* sreal,
                          double* g0mats, double* g0real, double* dmats, double* dreal, double* samats,
                          double* sareal, double* f0mats, double* f0real, void* stream) {
  SigmaArrays A;
  A.g[0] = (const SigC*)gm, A.g[1] = (const SigC*)gr;
  A.f[0] = (const SigC*)fm, A.f[1] = (const SigC*)fr;
  A.s[0] = (SigC*)smats, A.s[1] = (SigC*)sreal;
  A.g0[0] = (SigC*)g0mats, A.g0[1] = (SigC*)g0real;
  A.d[0] = (SigC*)dmats, A.d[1] = (SigC*)dreal;
  A.sa[0] = (SigC*)samats, A.sa[1] = (SigC*)sareal;
  A.f0[0] = (SigC*)f0mats, A.f0[1] = (SigC*)f0real;
  const char* why = "";
  auto* tab = new std::vector<SigmaBlock>();
  const int rc = sigma_compile(nblk, blocks, nspin, norb, beta, lmats, wini, wfin, lreal, A, tab, &why);
  if (rc != ED_OK) {
    delete tab;
    return fail(rc, std::string("ed_sigma_build: ") + why);
  }
  const bool with_g = gm || gr;
  bool nambu = false, has[kSigMaxN + 1] = {};
  for (const SigmaBlock& B : *tab) nambu = nambu || B.nambu, has[B.n] = true;
  hipStream_t st = (hipStream_t)stream;
  const size_t ncomp = (size_t)nspin * nspin * norb * norb, bytes = tab->size() * sizeof(SigmaBlock);
  const int nb = (int)tab->size();
  void* d = nullptr;
  hipError_t e = hipMallocAsync(&d, bytes, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d, tab->data(), bytes, hipMemcpyHostToDevice, st);
  // the staging table lives until the stream has passed the copy (no host
  // wait); from here on it belongs to free_staging and is not read again
  if (e != hipSuccess || hipLaunchHostFunc(st, free_staging, tab) != hipSuccess) {
    (void)hipStreamSynchronize(st);
    delete tab;
    if (d) (void)hipFreeAsync(d, st);
    return fail(ED_ERR_HIP, std::string("ed_sigma_build: table upload -> ") + hipGetErrorString(e));
  }
  // zero outside the blocks
  for (int ax = 0; ax < 2 && e == hipSuccess; ax++) {
    const size_t nbytes = ncomp * (size_t)(ax ? lreal : lmats) * sizeof(SigC);
    if (!nbytes) continue;
    SigC* out[5] = {with_g ? A.s[ax] : nullptr, A.g0[ax], A.d[ax], with_g && nambu ? A.sa[ax] : nullptr,
                    nambu ? A.f0[ax] : nullptr};
    for (SigC* o : out)
      if (o && e == hipSuccess) e = hipMemsetAsync(o, 0, nbytes, st);
  }
  if (e == hipSuccess) {
    const SigmaBlock* db = (const SigmaBlock*)d;
    const int wg = with_g ? 1 : 0;
    if (has[1]) launch_sigma<1>(nb, db, A, beta, lmats, wini, wfin, lreal, eps, wg, st);
    if (has[2]) launch_sigma<2>(nb, db, A, beta, lmats, wini, wfin, lreal, eps, wg, st);
    if (has[3]) launch_sigma<3>(nb, db, A, beta, lmats, wini, wfin, lreal, eps, wg, st);
    if (has[4]) launch_sigma<4>(nb, db, A, beta, lmats, wini, wfin, lreal, eps, wg, st);
    if (has[6]) launch_sigma<6>(nb, db, A, beta, lmats, wini, wfin, lreal, eps, wg, st);
    e = hipGetLastError();
  }
  (void)hipFreeAsync(d, st);
  if (e != hipSuccess) return fail(ED_ERR_HIP, std::string("ed_sigma_build -> ") + hipGetErrorString(e));
  return ED_OK;
}

int ed_sigma_build(const ed_params* p, double beta, int32_t lmats, double wini, double wfin, int32_t lreal,
                   double eps, const double* gm, const double* gr, const double* fm, const double* fr, double* smats,
                   double* sreal, double* g0mats, double* g0real, double* dmats, double* dreal, double* samats,
                   double* sareal, double* f0mats, double* f0real, void* stream) {
  std::vector<ed_sigma_block> blk(kSigMaxBlocks);
  int32_t nblk = 0;
  CK(ed_sigma_blocks(p, blk.data(), &nblk));
  return ed_sigma_build_blocks(nblk, blk.data(), p->nspin, p->norb, beta, lmats, wini, wfin, lreal, eps, gm, gr, fm,
                               fr, smats, sreal, g0mats, g0real, dmats, dreal, samats, sareal, f0mats, f0real, stream);
}
