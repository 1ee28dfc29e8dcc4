"""The host half of the self-energy kernel (csrc/ed_sigma_host.hpp) through a
stand-alone g++ driver (test infrastructure only): nothing of it is loaded into
Python, so the same driver also runs under AddressSanitizer + UBSan.

  build(dir, extra)   compile the driver (extra: more compiler flags).
  blocks_of(exe, cfg) sigma_blocks of a config -> (rc, ctypes array, count).
  run(exe, ...)       sigma_compile + sigma_host on given blocks and inputs.
  alias_codes(exe)    sigma_compile's answers to aliased arguments.
"""
import ctypes
import os
import subprocess

import numpy as np

from edgpu.sigma import SigmaBlock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmft-ed_amd", "csrc")
OUT_KEYS = ("s", "g0", "d", "sa", "f0")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "ed_sigma_host.hpp"
using namespace edg;
static bool slurp(const char* path, void* dst, size_t n) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(dst, 1, n, f) == n;
  fclose(f);
  return ok;
}
static bool dump(const char* path, const void* src, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(src, 1, n, f) == n;
  fclose(f);
  return ok;
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "blocks" && argc == 4) {   // params.bin blocks_out.bin
    ed_params p;
    if (!slurp(argv[2], &p, sizeof p)) return 3;
    std::vector<ed_sigma_block> blk(kSigMaxBlocks);
    int n = 0;
    const char* why = "";
    const int rc = sigma_blocks(p, blk.data(), &n, &why);
    printf("%d %d %s\n", rc, rc == ED_OK ? n : 0, why);
    if (rc == ED_OK && !dump(argv[3], blk.data(), (size_t)n * sizeof(ed_sigma_block))) return 3;
    return 0;
  }
  if (mode == "run" && argc == 15) {
    // blocks.bin nblk nspin norb beta lmats wini wfin lreal eps g.bin|- f.bin|- out.bin
    const int nblk = atoi(argv[3]), nspin = atoi(argv[4]), norb = atoi(argv[5]);
    const double beta = strtod(argv[6], nullptr), wini = strtod(argv[8], nullptr), wfin = strtod(argv[9], nullptr);
    const int lmats = atoi(argv[7]), lreal = atoi(argv[10]);
    const double eps = strtod(argv[11], nullptr);
    std::vector<ed_sigma_block> blk(nblk > 0 ? nblk : 1);
    if (nblk > 0 && !slurp(argv[2], blk.data(), (size_t)nblk * sizeof(ed_sigma_block))) return 3;
    const size_t ncomp = (size_t)nspin * nspin * norb * norb, nm = ncomp * lmats, nr = ncomp * lreal;
    const bool wg = strcmp(argv[12], "-") != 0, wf = strcmp(argv[13], "-") != 0;
    std::vector<SigC> g(nm + nr), f(nm + nr), out(5 * (nm + nr), SigC{0.0, 0.0});
    if (wg && !slurp(argv[12], g.data(), g.size() * sizeof(SigC))) return 3;
    if (wf && !slurp(argv[13], f.data(), f.size() * sizeof(SigC))) return 3;
    SigmaArrays A{};
    if (wg) A.g[0] = g.data(), A.g[1] = g.data() + nm;
    if (wf) A.f[0] = f.data(), A.f[1] = f.data() + nm;
    SigC* o = out.data();
    SigC** dst[5] = {A.s, A.g0, A.d, A.sa, A.f0};
    for (int k = 0; k < 5; k++) {
      dst[k][0] = o, dst[k][1] = o + nm;
      o += nm + nr;
    }
    std::vector<SigmaBlock> tab;
    const char* why = "";
    const int rc = sigma_compile(nblk, blk.data(), nspin, norb, beta, lmats, wini, wfin, lreal, A, &tab, &why);
    printf("%d %s\n", rc, why);
    if (rc != ED_OK) return 0;
    sigma_host(tab, A, beta, lmats, wini, wfin, lreal, eps);
    return dump(argv[14], out.data(), out.size() * sizeof(SigC)) ? 0 : 3;
  }
  if (mode == "alias") {
    // one n = 1 block on a 4-point Matsubara grid; each line one way of sharing bytes
    ed_sigma_block b{};
    b.n = 1, b.np = 1, b.e[0] = 0.5, b.c[0][0] = 1.0, b.w[0][0][0] = 0.3;
    std::vector<SigC> buf(64, SigC{1.0, 0.5});
    SigC* q = buf.data();
    for (int k = 0; k < 6; k++) {
      SigmaArrays A{};
      A.g[0] = q, A.s[0] = q + 8, A.g0[0] = q + 16, A.d[0] = q + 24;
      if (k == 1) A.s[0] = q;           // Sigma on G
      if (k == 2) A.g0[0] = q + 3;      // G0 overlapping G's tail
      if (k == 3) A.d[0] = q + 16;      // Delta on G0
      if (k == 4) A.d[0] = q + 9;       // Delta inside Sigma
      if (k == 5) A.g0[0] = q + 4;      // G0 next to G: no shared byte
      std::vector<SigmaBlock> tab;
      const char* why = "";
      const int rc = sigma_compile(1, &b, 1, 1, 10.0, 4, -1.0, 1.0, 0, A, &tab, &why);
      printf("%d %s\n", rc, why);
    }
    return 0;
  }
  return 2;
}
"""


def build(dirpath, extra=()):
    src = dirpath / "sigma_driver.cpp"
    src.write_text(DRIVER)
    exe = dirpath / ("sigma_driver" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", *extra, "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


def _run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    return out.stdout


def blocks_of(exe, cfg, dirpath, tag="m"):
    """(rc, message, ctypes array of ed_sigma_block, count) of sigma_blocks(cfg)."""
    pfile, bfile = dirpath / f"{tag}_params.bin", dirpath / f"{tag}_blocks.bin"
    pfile.write_bytes(bytes(cfg.to_ctypes()))
    f = _run([exe, "blocks", str(pfile), str(bfile)]).split(None, 2)
    rc, n = int(f[0]), int(f[1])
    if rc != 0:
        return rc, (f[2].strip() if len(f) > 2 else ""), None, 0
    raw = bfile.read_bytes()
    assert len(raw) == n * ctypes.sizeof(SigmaBlock)
    arr = (SigmaBlock * n).from_buffer_copy(raw)
    return rc, "", arr, n


def run(exe, dirpath, blocks, nspin, norb, beta, lmats, wini, wfin, lreal, eps, G=None, F=None, tag="r"):
    """(rc, message, outputs): outputs[key] = (mats, real) arrays (Nspin, Nspin,
    Norb, Norb, L) for key in OUT_KEYS, None when refused."""
    bfile, ofile = dirpath / f"{tag}_blocks.bin", dirpath / f"{tag}_out.bin"
    bfile.write_bytes(bytes(blocks))
    names = []
    for key, pair in (("g", G), ("f", F)):
        if pair is None:
            names.append("-")
            continue
        path = dirpath / f"{tag}_{key}.bin"
        path.write_bytes(b"".join(np.ascontiguousarray(a, dtype=np.complex128).tobytes() for a in pair))
        names.append(str(path))
    line = _run([exe, "run", str(bfile), str(len(blocks)), str(nspin), str(norb), float(beta).hex(), str(lmats),
                 float(wini).hex(), float(wfin).hex(), str(lreal), float(eps).hex(), names[0], names[1], str(ofile)])
    f = line.split(None, 1)
    rc = int(f[0])
    if rc != 0:
        return rc, (f[1].strip() if len(f) > 1 else ""), None
    raw = np.frombuffer(ofile.read_bytes(), dtype=np.complex128)
    shape = (nspin, nspin, norb, norb)
    ncomp = nspin * nspin * norb * norb
    out, at = {}, 0
    for key in OUT_KEYS:
        m = raw[at:at + ncomp * lmats].reshape(shape + (lmats,))
        r = raw[at + ncomp * lmats:at + ncomp * (lmats + lreal)].reshape(shape + (lreal,))
        out[key] = (m.copy(), r.copy())
        at += ncomp * (lmats + lreal)
    return rc, "", out


def alias_codes(exe):
    return [ln.split(None, 1) for ln in _run([exe, "alias"]).strip().split("\n")]
