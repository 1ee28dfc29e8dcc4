"""Superconducting Green's function (build_gf_superc / lanc_build_gf_superc_c,
ED_GF_SUPERC.f90:18-77, 88-446) on the CPU: the job list, build_gf_superc
through the oracle job runner of oracle_gf_superc against the dense direct sum
of superc_truth, and the host half of the mixed-operator seed kernel
(csrc/ed_seed_plan.hpp) through a stand-alone C++ driver.

Bars.  G(iw) and F(iw): 1e-10 of max(|G|, |F|), the project's bar.  G(w) and
F(w): the project's 1e-5.  The runner is the reference's plain Lanczos without
reorthogonalisation over the whole of these tiny sectors (nlanc = dim), so the
real-axis distance is that recurrence's own round-off weighed by 1/eps^2.
Measured with this file's replay (max over G and F of |replay - truth| /
max(|G|, |F|); Lreal = 32 on [-5, 5], T = 0 lists from the dense ground
states):

    eps     S1         S2         SH
    0.01    4.9e-14    7.4e-06    1.4e-05
    0.1     2.1e-14    3.9e-08    3.1e-07
    0.2     1.3e-14    6.2e-11    7.6e-10
    0.3     8.9e-15    2.1e-13    2.7e-12
    0.5     5.2e-15    3.8e-15    4.6e-15

Each model is checked at the smallest listed eps at which the replay holds
1e-5 (superc_truth.EPS: S1 0.01, S2 0.01, SH 0.1); the bar stays.  On the
Matsubara axis the replay is within 8.0e-15 (S1), 6.7e-14 (S2), 1.3e-14 (SH)
of the truth, and 5.1e-15 for the thermal S1 list (7 states, 2 twin entries).
"""
import os
import subprocess

import numpy as np
import pytest

import superc_truth as st
from edgpu.diag import DiagOptions, StateList, post_diag, state_list
from edgpu.gf import GFOptions, _job_list_superc, build_gf, build_gf_superc, matsubara, realaxis
from edgpu.sectors import get_sector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmft-ed_amd", "csrc")
MODELS = ["S1", "S2", "SH"]


def gopt(name, **kw):
    return GFOptions(Lmats=32, Lreal=32, eps=st.EPS[name], **kw)


def ground_list(name):
    """The T = 0 list of the dense eigenpairs (two per sector are enough for the window)."""
    T = st.truth(name)
    return state_list(T.sector_results(2), DiagOptions(), T.cfg)


def one_state_list(cfg, sz):
    sec = get_sector(cfg)[(sz, 0)]
    v = np.zeros(sec.dim)
    v[0] = 1.0
    return StateList([0.0], [sec.isector], [v])


def test_build_gf_names_the_superc_function():
    cfg = st.config("S1")
    with pytest.raises(NotImplementedError, match="build_gf_superc"):
        build_gf(cfg, one_state_list(cfg, 0), GFOptions(Lmats=4, Lreal=4))
    from edgpu.params import make_config

    ncfg = make_config(Norb=1, Nbath=2)
    with pytest.raises(ValueError):
        build_gf_superc(ncfg, StateList([0.0], [1], [np.ones(1)]), GFOptions(Lmats=4, Lreal=4))


def test_job_list_of_a_state_in_sz0():
    cfg = st.config("S2")
    Ns = cfg.Ns
    jobs = _job_list_superc(cfg, one_state_list(cfg, 0))
    assert len(jobs) == 12
    at = 0
    for a in range(cfg.Norb):
        up, dw = a, a + Ns
        want = [(0, [(up, 1, 1)], +1, +1), (0, [(up, 1, 0)], -1, -1),              # G_aa:    c+_up, c_up
                (1, [(dw, 1, 0)], +1, +1), (1, [(dw, 1, 1)], -1, -1),              # barG_aa: c_dw, c+_dw
                (2, [(up, 1, 1), (dw, 1, 0)], +1, +1), (2, [(up, 1, 0), (dw, 1, 1)], -1, -1)]   # A_aa
        for chan, terms, isign, dsz in want:
            comp, tag, k, (op, sg, ispin, tt, weight), src, dst = jobs[at]
            assert comp == 3 * a + chan and tag == ("superc", chan, a) and k == 0
            assert tt == terms and op == terms[0][2] and sg == isign and weight == 1.0
            assert src.q1 == 0 and dst.q1 == dsz
            at += 1


@pytest.mark.parametrize("sz,isign", [(+1, -1), (-1, +1)])
def test_job_list_at_the_end_sectors(sz, isign):
    """A state in sz = +-Ns has one target sector: three seeds per orbital are left."""
    cfg = st.config("S2")
    jobs = _job_list_superc(cfg, one_state_list(cfg, sz * cfg.Ns))
    assert len(jobs) == 3 * cfg.Norb
    assert all(j[3][1] == isign and j[5].q1 == sz * (cfg.Ns - 1) for j in jobs)
    assert [j[0] for j in jobs] == list(range(3 * cfg.Norb))


def test_job_order_is_orbital_then_state_then_seed():
    cfg = st.config("S2")
    a, b = get_sector(cfg)[(0, 0)], get_sector(cfg)[(1, 0)]
    sl = StateList([0.0, 0.0], [a.isector, b.isector], [np.ones(a.dim), np.ones(b.dim)])
    jobs = _job_list_superc(cfg, sl)
    assert [(j[0] // 3, j[2]) for j in jobs] == [(o, k) for o in range(2) for k in range(2) for _ in range(6)]


@pytest.mark.parametrize("name", MODELS)
def test_g_and_f_match_the_dense_truth(name):
    from oracle_gf_superc import oracle_job_runner_superc

    T, g = st.truth(name), gopt(name)
    cfg, sl = T.cfg, ground_list(name)
    wm, wr = matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal)
    got = build_gf_superc(cfg, sl, g, runner=oracle_job_runner_superc)
    tr = T.gf_of_list(sl, wm, wr, g.eps)
    dm, dr, ratio = st.distances(tr, got, wm, wr, g.eps)
    gbar = np.max(np.abs(tr["G"][0] - tr["Gbar"][0])) / np.max(np.abs(tr["G"][0]))
    print(f"{name}: {sl.size} state(s) in sz {[T.sz_of[i] for i in sl.sectors]}, eps {g.eps}: (iw) {dm:.2e}, "
          f"(w) {dr:.2e}; truth max|F|/max|G| {ratio:.3f}, max|G - barG|/max|G| {gbar:.3f}")
    for arr in got:
        assert arr.shape == (1, 1, cfg.Norb, cfg.Norb, 32) and arr.dtype == np.complex128
    assert ratio > 0.05                       # F is not small: the recombination is exercised
    if name == "S1":
        assert gbar > 0.05                    # xmu != 0: G and barG differ, the three channels are distinct
    assert dm < 1e-10 and dr < 1e-5
    for arr in got:                           # orbital off-diagonal entries are not built: exactly zero
        for a in range(cfg.Norb):
            for b in range(cfg.Norb):
                if a != b:
                    assert not np.any(arr[0, 0, a, b])
                else:
                    assert np.any(arr[0, 0, a, a])


def thermal_list():
    T = st.truth("S1")
    opt = DiagOptions(lanc_nstates_total=st.NTOTAL, beta=st.BETA, cutoff=st.CUTOFF, ed_twin=True)
    sl, _ = post_diag(state_list(T.sector_results(6, True), opt, T.cfg), opt, T.cfg)
    return sl


def test_thermal_list_with_twin_entries():
    from oracle.oracle import Oracle
    from oracle_gf_superc import host_state_vector, oracle_job_runner_superc

    T = st.truth("S1")
    cfg, sl = T.cfg, thermal_list()
    kept = T.thermal_states()
    per_sector = max(sum(1 for t in kept if t[1] == i) for i in {t[1] for t in kept})
    assert sl.size == len(kept) and per_sector < 6 and sum(p is not None for p in sl.twin_of) >= 1
    # a twin vector is an eigenvector only with superc_twin_sign
    orc, worst, bare = Oracle(cfg), 0.0, 0.0
    for k, p in enumerate(sl.twin_of):
        if p is None:
            continue
        idx = T.maps[sl.sectors[k]]
        blk = T.H[idx][:, idx].toarray()
        res = lambda v: np.linalg.norm(blk @ v - sl.energies[k] * v)    # noqa: E731
        worst = max(worst, res(host_state_vector(cfg, orc, sl, k)))
        bare = max(bare, res(host_state_vector(cfg, orc, sl, k, sign=False)))
    print(f"twin vectors: |(H - E) v| {worst:.2e} with the sign, {bare:.2e} without")
    assert worst < 1e-12 and bare > 0.1
    g = gopt("S1", beta=st.BETA)
    wm, wr = matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal)
    got = build_gf_superc(cfg, sl, g, runner=oracle_job_runner_superc)
    dm, dr, ratio = st.distances(T.gf_thermal(wm, wr, g.eps), got, wm, wr, g.eps)
    print(f"thermal S1: {sl.size} states, {sum(p is not None for p in sl.twin_of)} twin entries: (iw) {dm:.2e}, "
          f"(w) {dr:.2e}; truth max|F|/max|G| {ratio:.3f}")
    assert ratio > 0.05 and dm < 1e-10 and dr < 1e-5
    with pytest.raises(ValueError, match="beta"):
        build_gf_superc(cfg, sl, gopt("S1"), runner=oracle_job_runner_superc)     # GFOptions.beta = 1000


def test_no_cut_at_large_beta_de():
    """add_to_lanczos_gf_superc has no beta (Ei - Egs) < 200 cut (ED_GF_SUPERC.f90:773-782):
    the weight is the plain Boltzmann factor where the normal-mode one is zero."""
    from edgpu.gf import _peso_bz, _peso_superc

    sl = StateList([0.0, 30.0], [1, 1], [None, None], finite_t=True, beta=10.0)
    assert _peso_bz(sl, 1, 1.0, 2.0, 1.0) == 0.0
    assert _peso_superc(sl, 1, 1.0, 2.0, 1.0) == 2.0 * np.exp(-300.0)
    assert _peso_superc(sl, 0, 1.0, 2.0, 4.0) == 0.5
    t0 = StateList([0.0, 0.0], [1, 2], [None, None])
    assert _peso_superc(t0, 1, 1.0, 3.0, 2.0) == 1.5


# ------------------------------------------------------------ the plan header on the host
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ed_seed_plan.hpp"
using namespace edg;
static FILE* in;
static std::string tok() {
  char b[128];
  if (fscanf(in, "%127s", b) != 1) return "";
  return b;
}
static long I() { return strtol(tok().c_str(), nullptr, 10); }
static double D() { return strtod(tok().c_str(), nullptr); }
int main(int argc, char** argv) {
  in = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!in) return 2;
  SeedSectors S{0, 0, 0, nullptr, 0, 0, 0, 0};
  std::vector<uint32_t> msrc, mdst;
  std::vector<double> x;
  int vc = 0;
  for (std::string c = tok(); !c.empty(); c = tok()) {
    if (c == "sectors") {       // ns mode src_q1 src_q2 dst_q1 dst_q2
      S.ns = (int)I(); S.mode = (int)I();
      S.src_q1 = (int)I(); S.src_q2 = (int)I(); S.dst_q1 = (int)I(); S.dst_q2 = (int)I();
    } else if (c == "maps") {   // dim_src states..., dim_dst states...
      msrc.resize(I());
      for (auto& m : msrc) m = (uint32_t)I();
      mdst.resize(I());
      for (auto& m : mdst) m = (uint32_t)I();
    } else if (c == "vec") {    // vc values...
      vc = (int)I();
      x.resize(msrc.size() * (vc ? 2 : 1));
      for (auto& v : x) v = D();
    } else if (c == "plan") {   // nlev levels ops nseed (p q)... run
      const int nlev = (int)I();
      std::vector<int32_t> lev(std::max(nlev, 1)), op(std::max(nlev, 1));
      for (int l = 0; l < nlev; l++) lev[l] = (int32_t)I();
      for (int l = 0; l < nlev; l++) op[l] = (int32_t)I();
      const int nseed = (int)I();
      std::vector<int32_t> terms(2 * std::max(nseed, 1));
      for (int s = 0; s < 2 * nseed; s++) terms[s] = (int32_t)I();
      const int run = (int)I();
      SeedPlan P;
      const int rc = seed_plan_compile(S, nlev, lev.data(), op.data(), nseed, terms.data(), &P);
      printf("%d", rc);
      if (rc == ED_OK && run) {
        const size_t w = vc ? 2 : 1, dim = mdst.size();
        std::vector<double> seeds((size_t)nseed * dim * w), n2(nseed);
        seed_plan_host(P, (int64_t)dim, mdst.data(), x.data(), vc != 0,
                       [&](uint32_t k) { return (int64_t)(std::lower_bound(msrc.begin(), msrc.end(), k) - msrc.begin()); },
                       seeds.data(), n2.data());
        for (double v : n2) printf(" %a", v);
        for (double v : seeds) printf(" %a", v);
      }
      printf("\n");
    } else {
      return 3;
    }
  }
  return 0;
}
"""


def _build(dirpath, extra=()):
    src = dirpath / "seed_plan_driver.cpp"
    src.write_text(DRIVER)
    exe = dirpath / ("seed_plan_driver" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", *extra, "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


def _plan_line(levels, ops, terms, run=1):
    flat = [t for pq in terms for t in pq]
    return "plan %d %s %s %d %s %d" % (len(levels), " ".join(map(str, levels)), " ".join(map(str, ops)), len(terms),
                                       " ".join(map(str, flat)), run)


def _numpy_seed(orc, hmap_i, jsec, terms, x):
    from oracle_gf import seed

    v = None
    for lv, o in terms:
        _, w = seed(orc, hmap_i, jsec, o, lv, x.astype(np.complex128))
        v = w if v is None else v + w
    return v


class _Cases:
    """The driver's input: S2, sz 0 -> +1 and 0 -> -1 (dims 70 -> 56), real and
    complex random vectors, the six images and nine seeds of both orbitals;
    then the plans that must be refused."""

    def __init__(self, dirpath):
        from edgpu.params import MODES
        from oracle.oracle import Oracle

        self.cfg = cfg = st.config("S2")
        self.orc = orc = Oracle(cfg)
        Ns = cfg.Ns
        self.lines, self.expect = [], []
        src = orc.build_sector(0, 0)
        rng = np.random.default_rng(11)
        for dsz in (+1, -1):
            dst = orc.build_sector(dsz, 0)
            assert (len(src), len(dst)) == (70, 56)
            self.lines.append(f"sectors {Ns} {MODES['superc']} 0 0 {dsz} 0")
            self.lines.append("maps %d %s %d %s" % (len(src), " ".join(str(int(m)) for m in src), len(dst),
                                                    " ".join(str(int(m)) for m in dst)))
            # raise sz: c+_up (op 1) and c_dw (op 0); lower sz: c_up and c+_dw
            ops = (1, 0) if dsz > 0 else (0, 1)
            levels = [0, Ns, 1, Ns + 1]
            lops = [ops[0], ops[1], ops[0], ops[1]]
            terms = [(0, -1), (1, -1), (0, 1), (2, -1), (3, -1), (2, 3), (1, 0), (0, 3), (3, 2)]
            for cplx in (False, True):
                x = rng.normal(size=len(src)) + (1j * rng.normal(size=len(src)) if cplx else 0.0)
                flat = np.ascontiguousarray(x).view(np.float64)
                self.lines.append("vec %d %s" % (int(cplx), " ".join(float(v).hex() for v in flat)))
                self.lines.append(_plan_line(levels, lops, terms))
                self.expect.append(("run", dsz, cplx, x, [(levels[p], lops[p]) for p in range(4)], terms))
            up, dn = ops
            bad = [
                ([0, Ns], [up, up], [(0, 1)]),                # c+_up with c+_dw: the second reaches the other sector
                ([0, 1], [1 - up, 1 - up], [(0, 1)]),         # both into the other target sector
                ([0, Ns, 0], [up, dn, up], [(0, 1)]),         # duplicate (level, op)
                ([0, Ns], [up, dn], [(1, 1)]),                # p = q
                ([0, Ns], [up, dn], [(0, 2)]),                # q >= nlev
                ([0, Ns], [up, dn], [(2, -1)]),               # p >= nlev
                ([0, Ns], [up, dn], [(-1, 0)]),               # p < 0
                ([2 * Ns, Ns], [up, dn], [(0, 1)]),           # level >= 2*Ns
                ([0, Ns], [2, dn], [(0, 1)]),                 # op outside {0, 1}
                ([], [], [(0, -1)]),                          # nlev = 0
                ([0], [up], []),                              # nseed = 0
                ([0], [up], [(0, -1)] * 33),                  # nseed = 33
            ]
            for lv, lo, tt in bad:
                self.lines.append(_plan_line(lv, lo, tt, run=0))
                self.expect.append(("bad",))
            good = [([0, Ns], [up, dn], [(0, 1)]), ([Ns], [dn], [(0, -1)]), ([0], [up], [(0, -1)] * 32)]
            for lv, lo, tt in good:
                self.lines.append(_plan_line(lv, lo, tt, run=0))
                self.expect.append(("good",))
        # nlev = 7 needs seven distinct images into one sector: Norb = 2 has four, so levels of the bath too
        self.lines.append(_plan_line([0, 1, 2, 3, Ns, Ns + 1, Ns + 2], [0, 0, 0, 0, 1, 1, 1], [(0, 1)], run=0))
        self.expect.append(("bad",))
        self.lines.append(_plan_line([0, 1, 2, 3, Ns, Ns + 1], [0, 0, 0, 0, 1, 1], [(0, 5)], run=0))
        self.expect.append(("good",))
        self.path = dirpath / "cases.txt"
        self.path.write_text("\n".join(self.lines) + "\n")


@pytest.fixture(scope="module")
def plan_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("seed_plan")
    c = _Cases(d)
    c.dir = d
    c.raw = subprocess.run([_build(d), str(c.path)], capture_output=True, text=True, check=True).stdout
    return c


def test_plan_validation_and_row_rule_on_the_host(plan_run):
    from edgpu.sectors import get_sector as gs

    c = plan_run
    rows = c.raw.strip().split("\n")
    assert len(rows) == len(c.expect)
    nrun = nbad = ngood = 0
    worst = worst_n = 0.0
    for row, exp in zip(rows, c.expect):
        f = row.split()
        if exp[0] == "bad":
            assert f == ["1"], (row[:40], exp)            # ED_ERR_ARG
            nbad += 1
        elif exp[0] == "good":
            assert f == ["0"]
            ngood += 1
        else:
            _, dsz, cplx, x, images, terms = exp
            assert f[0] == "0"
            vals = np.array([float.fromhex(t) for t in f[1:]])
            n2, seeds = vals[:len(terms)], vals[len(terms):]
            seeds = seeds.view(np.complex128) if cplx else seeds
            seeds = seeds.reshape(len(terms), 56)
            hmap_i = c.orc.build_sector(0, 0)
            jsec = gs(c.cfg)[(dsz, 0)]
            for s, (p, q) in enumerate(terms):
                ref = _numpy_seed(c.orc, hmap_i, jsec, [images[p]] + ([images[q]] if q >= 0 else []), x)
                if not cplx:
                    assert np.max(np.abs(ref.imag)) == 0.0
                assert np.any(ref != 0)
                # one product and at most one addition per element, in the numpy seed's order: the same bits
                worst = max(worst, np.max(np.abs(seeds[s] - (ref if cplx else ref.real))))
                worst_n = max(worst_n, abs(n2[s] - np.vdot(ref, ref).real) / np.vdot(ref, ref).real)
            nrun += 1
    print(f"{nrun} runs of 9 seeds: max |host - numpy| {worst:.2e}, norm2 {worst_n:.2e}; {nbad} plans refused, "
          f"{ngood} accepted")
    assert nrun == 4 and nbad == 25 and ngood == 7
    assert worst == 0.0 and worst_n < 1e-14


def test_driver_clean_under_sanitizers(plan_run):
    """The same driver and cases under AddressSanitizer + UBSan (host code with
    its own main): no report, same output."""
    exe = _build(plan_run.dir, ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe, str(plan_run.path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    assert out.stdout == plan_run.raw
