"""Spin and density susceptibilities (edgpu.chi, buildChi_impurity
ED_GREENS_FUNCTIONS.f90:72-106) on the CPU: the host half of the diagonal
seed kernel (csrc/ed_chi_host.hpp) through a stand-alone C++ driver, the job
and component layout, the static term, and the whole chain in numpy
(chi_host.replay_chi) against the dense Lehmann sums of chi_truth.

Bars.  chi(iv) and chi(tau): 1e-10 of each array's maximum.  chi(w): the
project's 1e-5.  The replay is the reference's plain Lanczos without
reorthogonalisation over the whole of these tiny sectors (nlanc = dim), so
the real-axis distance is that recurrence's own round-off weighed by 1/eps^2.
Measured with this file's replay (max over all compared components of
|replay - truth| / max|truth array|; Lmats = 32, Ltau = 24, Lreal = 32 on
[-5, 5], beta = 8, T = 0 lists from the dense ground states):

    eps     C1         C2         CN         thermal C1
    0.01    8.5e-15    1.8e-14    1.5e-07    2.2e-14
    0.1     4.6e-15    1.5e-14    3.5e-09    1.0e-14
    0.2     3.5e-15    1.4e-14    2.4e-11    7.1e-15
    0.3     2.7e-15    1.4e-14    2.3e-13    5.2e-15
    0.5     2.3e-15    1.5e-14    1.8e-15    3.3e-15

Every model holds 1e-5 at the smallest listed eps, 0.01 (chi_truth.EPS), and
the GPU test uses it.  On the other two grids the replay is within 2.7e-15 /
3.0e-15 (C1: iv / tau), 6.0e-15 / 6.0e-15 (C2, 3 degenerate states),
4.9e-15 / 4.1e-15 (CN, complex vectors) and 1.6e-15 / 2.5e-15 (thermal C1, 7
states, 2 twin entries) of the truth.  The smallest share of an array that
comes from poles with |D| > 1e-6: C1 4.3e-3, C2 2.3e-3 (the density cross
term on iv), CN 1.4e-3, thermal 4.5e-3; chi_truth asserts >= 1e-3.
"""
import os
import subprocess

import numpy as np
import pytest

import chi_truth as ct
from chi_host import chi_poles_host, numpy_seeds, replay_chi, thermal_host
from edgpu import chi
from edgpu.diag import DiagOptions, StateList, post_diag, state_list
from edgpu.params import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmft-ed_amd", "csrc")
MODELS = ["C1", "C2", "CN"]


def ground_list(name):
    """The T = 0 list of the dense eigenpairs (two per sector are enough for the window)."""
    T = ct.truth(name)
    return state_list(T.sector_results(2), DiagOptions(), T.cfg)


def thermal_list():
    T = ct.truth("C1")
    opt = DiagOptions(lanc_nstates_total=ct.NTOTAL, beta=ct.BETA, cutoff=ct.CUTOFF, ed_twin=True)
    sl, _ = post_diag(state_list(T.sector_results(6, True), opt, T.cfg), opt, T.cfg)
    return sl


# ------------------------------------------------------------ layout
def test_exported_from_the_package():
    import edgpu

    assert edgpu.build_chi is chi.build_chi and edgpu.ChiOptions is chi.ChiOptions


def test_options_and_grids():
    o = chi.ChiOptions()
    assert (o.lanc_nGFiter, o.Lmats, o.Lreal, o.Ltau) == (200, 5000, 5000, 1000)
    assert o.ltau == 1000 and chi.ChiOptions(beta=8.0, Ltau=4).ltau == 8 and chi.ChiOptions(beta=8.7, Ltau=24).ltau == 24
    vm = chi.bosonic_matsubara(8.0, 5)
    assert vm.shape == (6,) and vm[0] == 0.0 and np.array_equal(vm, np.pi / 8.0 * 2.0 * np.arange(6))
    tg = chi.tau_grid(8.0, 16)
    assert tg.shape == (17,) and tg[0] == 0.0 and tg[-1] == 8.0


def test_seed_table_norb1_has_no_totals():
    cfg = ct.config("C1")
    Ns = cfg.Ns
    assert chi.seed_levels(cfg) == [0, Ns]
    t = chi.seed_table(cfg)
    assert [n for n, _, _ in t] == [("spin", 0), ("dens", 0)]
    assert [c for _, c, _ in t] == [0, 2] and chi.n_components(cfg) == 4
    assert np.array_equal(t[0][2], [0.5, -0.5]) and np.array_equal(t[1][2], [1.0, 1.0])
    assert [n for n, _, _ in chi.seed_table(cfg, spin=False)] == [("dens", 0)]
    assert [n for n, _, _ in chi.seed_table(cfg, dens=False)] == [("spin", 0)]


def test_seed_table_norb3_is_eleven_seeds_over_six_levels():
    cfg = make_config(Norb=3, Nbath=1)
    Ns = cfg.Ns
    assert chi.seed_levels(cfg) == [0, 1, 2, Ns, Ns + 1, Ns + 2]
    t = chi.seed_table(cfg)
    names = [n for n, _, _ in t]
    assert names == [("spin", 0), ("spin", 1), ("spin", 2), ("spin_tot",), ("dens", 0), ("dens", 1), ("dens", 2),
                     ("dens_pair", 0, 1), ("dens_pair", 0, 2), ("dens_pair", 1, 2), ("dens_tot",)]
    assert [c for _, c, _ in t] == list(range(11)) and chi.n_components(cfg) == 11
    w = {n: v for n, _, v in t}
    assert np.array_equal(w[("spin", 1)], [0, 0.5, 0, 0, -0.5, 0])
    assert np.array_equal(w[("spin_tot",)], [0.5, 0.5, 0.5, -0.5, -0.5, -0.5])
    assert np.array_equal(w[("dens", 2)], [0, 0, 1, 0, 0, 1])
    assert np.array_equal(w[("dens_pair", 0, 2)], [1, 0, 1, 1, 0, 1])
    assert np.array_equal(w[("dens_tot",)], [1] * 6)
    # the components do not move when a part is left out
    assert [c for _, c, _ in chi.seed_table(cfg, spin=False)] == list(range(4, 11))
    assert [c for _, c, _ in chi.seed_table(cfg, dens=False)] == list(range(4))


def test_job_order_is_state_then_seed():
    cfg = ct.config("C2")
    sl = StateList([0.0, 0.0, 0.0], [9, 13, 17], [None, None, None])
    jobs = chi.chi_jobs(cfg, sl)
    n = len(chi.seed_table(cfg))
    assert n == 7 and len(jobs) == 3 * n
    assert [(k, q) for k, q, _, _ in jobs] == [(k, q) for k in range(3) for q in range(n)]
    assert [name for _, _, name, _ in jobs[:n]] == [("spin", 0), ("spin", 1), ("spin_tot",), ("dens", 0), ("dens", 1),
                                                    ("dens_pair", 0, 1), ("dens_tot",)]


def test_recombination_indices():
    cfg = make_config(Norb=3, Nbath=1)
    copt = chi.ChiOptions(Lmats=2, Ltau=3, Lreal=4, beta=2.0)
    nc = chi.n_components(cfg)
    val = np.array([1.0, 2.0, 3.0, 4.0, 10.0, 20.0, 40.0, 37.0, 56.0, 72.0, 99.0])      # per flat component
    iv = (val[:, None] * (1 + 2j)) * np.ones((nc, 3))
    tau = val[:, None] * np.ones((nc, 4))
    w = (val[:, None] * (3 - 1j)) * np.ones((nc, 4))
    c = chi.assemble(cfg, copt, iv, tau, w)
    assert c.spin_iv.shape == (4, 3) and c.spin_tau.shape == (4, 4) and c.spin_w.shape == (4, 4)
    assert c.dens_iv.shape == (3, 3, 3) and c.dens_tau.shape == (3, 3, 4) and c.dens_tot_w.shape == (4,)
    assert np.array_equal(c.spin_tau[:, 0], [1, 2, 3, 4]) and np.all(c.dens_tot_tau == 99.0)
    want = np.array([[10.0, 0.5 * (37 - 10 - 20), 0.5 * (56 - 10 - 40)],
                     [0.5 * (37 - 10 - 20), 20.0, 0.5 * (72 - 20 - 40)],
                     [0.5 * (56 - 10 - 40), 0.5 * (72 - 20 - 40), 40.0]])
    assert np.array_equal(c.dens_tau[:, :, 1], want)
    assert np.array_equal(c.dens_iv[:, :, 2], want * (1 + 2j)) and np.array_equal(c.dens_w[:, :, 0], want * (3 - 1j))
    only = chi.assemble(cfg, copt, iv, tau, w, spin=False)
    assert only.spin_iv is None and np.array_equal(only.dens_tau, c.dens_tau)


def test_refusals(monkeypatch):
    class World:
        @staticmethod
        def get_world_size():
            return 2

    with monkeypatch.context() as m:
        m.setattr(chi, "_dist", lambda: World)
        with pytest.raises(NotImplementedError, match="rank split"):
            chi.build_chi(ct.config("C1"), StateList([0.0], [1], [np.ones(1)]), chi.ChiOptions(Lmats=4, Lreal=4, Ltau=4))
    sc = make_config(Norb=1, Nbath=2, ed_mode="superc", deltasc=0.3)
    with pytest.raises(NotImplementedError, match="superc"):
        chi.build_chi(sc, StateList([0.0], [1], [np.ones(1)]), chi.ChiOptions(Lmats=4, Lreal=4, Ltau=4))
    sl = StateList([0.0], [1], [np.ones(1)], finite_t=True, beta=8.0)
    with pytest.raises(ValueError, match="beta"):
        chi.build_chi(ct.config("C1"), sl, chi.ChiOptions(Lmats=4, Lreal=4, Ltau=4))     # ChiOptions.beta = 1000


# ------------------------------------------------------------ the static term (departure 1)
def test_static_term_is_continuous_and_right_below_zero():
    beta = 8.0
    cut = 0.1 / beta                                     # the reference switches to beta at beta*D < 0.1
    below, above = np.nextafter(cut, 0.0), np.nextafter(cut, 1.0)
    _, s = thermal_host(beta, np.array([below, cut, above, 0.0, 1e-300, -1e-12, 1e-12, -0.5, -2.0]))
    assert abs(s[0] - s[2]) < 1e-14 * s[1]               # no jump at the cut (the reference's is 4.8 %)
    assert abs(s[1] - beta) / beta > 0.04                # ... which the reference's value beta misses by that much
    exact = (1.0 - np.exp(-0.1)) / cut
    assert abs(s[1] - exact) < 2e-15 * exact             # 1 - exp(-0.1) itself carries 1.1e-16 / 0.095
    assert s[3] == beta and abs(s[4] - beta) < 1e-15 * beta
    assert abs(s[5] - beta) < 1e-10 * beta and abs(s[6] - beta) < 1e-10 * beta
    # D < 0 (a downward transition of a thermal state): (exp(beta |D|) - 1) / |D|, not beta
    for k, D in ((7, -0.5), (8, -2.0)):
        want = (np.exp(beta * -D) - 1.0) / -D
        assert abs(s[k] - want) < 1e-15 * want and s[k] > 3.0 * beta
    # and it is what the pole sum puts at iv(0): one pole, weight 1, both isign terms
    for D in (below, above, -0.5):
        iv, _, _, _ = chi_poles_host([(0, 1.0, 0.0, [D], [1.0])], beta, chi.bosonic_matsubara(beta, 2),
                                     chi.tau_grid(beta, 2), np.zeros(1), 0.1, 1)
        assert iv[0, 0] == 2.0 * thermal_host(beta, D)[1]


def test_pole_sum_of_one_pole_by_hand():
    beta, D, eps = 8.0, 0.3, 0.05
    vm, tg, wr = chi.bosonic_matsubara(beta, 3), chi.tau_grid(beta, 4), np.array([-1.0, 0.2])
    iv, tau, w, mag = chi_poles_host([(1, 0.5, -1.0, [-1.0 + D], [0.6])], beta, vm, tg, wr, eps, 2)
    p, f = 0.5 * 0.36, 1.0 - np.exp(-beta * D)
    assert not np.any(iv[0]) and not np.any(tau[0]) and not np.any(w[0])
    assert abs(iv[1, 0] - 2 * p * f / D) < 1e-14
    np.testing.assert_allclose(iv[1, 1:], p * f * (1 / (1j * vm[1:] + D) - 1 / (1j * vm[1:] - D)), rtol=1e-14)
    np.testing.assert_allclose(tau[1], p * (np.exp(-tg * D) + np.exp(-(beta - tg) * D)), rtol=1e-14)
    np.testing.assert_allclose(w[1], p * f * (1 / (wr + 1j * eps + D) - 1 / (wr + 1j * eps - D)), rtol=1e-14)
    assert np.all(mag[1][1] >= np.abs(tau[1]))


# ------------------------------------------------------------ the chain against the dense truth
@pytest.mark.parametrize("name", MODELS)
def test_replay_matches_the_dense_truth(name):
    T, copt, sl = ct.truth(name), ct.options(name), ground_list(name)
    cfg = T.cfg
    rec = []
    got = replay_chi(cfg, sl, copt, record=rec)
    d = ct.distances(T.chi_of_list(sl, copt), got, cfg.Norb)
    print(f"{name}: {sl.size} state(s) in sectors {sl.sectors}, eps {copt.eps}: iv {d[0]:.2e}, tau {d[1]:.2e}, "
          f"w {d[2]:.2e}; smallest dynamic share {min(T.shares.values()):.2e}")
    if name == "CN":
        assert all(np.iscomplexobj(v) for v in sl.vectors)
    assert [(r["state"], r["name"]) for r in rec] == [(k, n) for k, _, n, _ in chi.chi_jobs(cfg, sl)]     # no seed vanished
    No = cfg.Norb
    assert got.spin_iv.shape == (No + 1, ct.LMATS + 1) and got.spin_tau.shape == (No + 1, ct.LTAU + 1)
    assert got.dens_w.shape == (No, No, ct.LREAL) and got.dens_tot_tau.shape == (ct.LTAU + 1,)
    if No == 1:
        assert not np.any(got.spin_iv[1]) and not np.any(got.spin_tau[1]) and not np.any(got.dens_tot_w)
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5
    # a part left out leaves the other as it is
    s_only, d_only = replay_chi(cfg, sl, copt, dens=False), replay_chi(cfg, sl, copt, spin=False)
    assert s_only.dens_iv is None and d_only.spin_w is None
    for a, b in ((s_only.spin_iv, got.spin_iv), (s_only.spin_tau, got.spin_tau), (d_only.dens_w, got.dens_w),
                 (d_only.dens_tot_tau, got.dens_tot_tau)):
        assert np.array_equal(a, b)


def test_replay_of_the_thermal_list_with_twin_entries():
    T, copt, sl = ct.truth("C1"), ct.options("C1"), thermal_list()
    kept = T.thermal_states()
    assert sl.finite_t and sl.size == len(kept) and sum(p is not None for p in sl.twin_of) >= 1
    assert len(set(sl.sectors)) < sl.size                 # a sector holds more than one kept state
    assert any(e > sl.emin + 0.05 for e in sl.energies)   # excited states: poles with D < 0
    got = replay_chi(T.cfg, sl, copt)
    d = ct.distances(T.chi_thermal(copt), got, 1)
    print(f"thermal C1: {sl.size} states, {sum(p is not None for p in sl.twin_of)} twin entries: iv {d[0]:.2e}, "
          f"tau {d[1]:.2e}, w {d[2]:.2e}")
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5


# ------------------------------------------------------------ the table header on the host
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ed_chi_host.hpp"
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
  int ns = 0, vc = 0;
  std::vector<uint32_t> map;
  std::vector<double> x;
  for (std::string c = tok(); !c.empty(); c = tok()) {
    if (c == "ns") {
      ns = (int)I();
    } else if (c == "map") {    // dim states...
      map.resize(I());
      for (auto& m : map) m = (uint32_t)I();
    } else if (c == "vec") {    // vc values...
      vc = (int)I();
      x.resize(map.size() * (vc ? 2 : 1));
      for (auto& v : x) v = D();
    } else if (c == "table") {  // nlev levels nseed weights[nseed][nlev] run
      const int nlev = (int)I();
      std::vector<int32_t> lev(std::max(nlev, 1));
      for (int l = 0; l < nlev; l++) lev[l] = (int32_t)I();
      const int nseed = (int)I();
      std::vector<double> w((size_t)std::max(nseed, 1) * std::max(nlev, 1));
      for (int k = 0; k < nseed * nlev; k++) w[k] = D();
      const int run = (int)I();
      DiagTable T;
      const int rc = seed_diag_compile(ns, nlev, lev.data(), nseed, w.data(), &T);
      printf("%d", rc);
      if (rc == ED_OK && run) {
        const size_t cw = vc ? 2 : 1, dim = map.size();
        std::vector<double> seeds((size_t)nseed * dim * cw), n2(nseed);
        seed_diag_host(T, (int64_t)dim, map.data(), x.data(), vc != 0, seeds.data(), n2.data());
        for (double v : n2) printf(" %a", v);
        for (double v : seeds) printf(" %a", v);
      }
      printf("\n");
    } else if (c == "thermal") {  // beta D
      const double beta = D(), de = D();
      double f, s;
      chi_thermal(beta, de, &f, &s);
      printf("%a %a\n", f, s);
    } else {
      return 3;
    }
  }
  return 0;
}
"""

THERMAL_D = [0.0, 1e-300, 1e-12, -1e-12, 0.0125, 0.3, 5.0, -0.5, -2.0, 200.0]


def _build(dirpath, extra=()):
    src = dirpath / "seed_diag_driver.cpp"
    src.write_text(DRIVER)
    exe = dirpath / ("seed_diag_driver" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", *extra, "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


def _table_line(levels, weights, run=1):
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    nseed = 0 if len(levels) == 0 and w.size == 0 else (len(weights))
    return "table %d %s %d %s %d" % (len(levels), " ".join(map(str, levels)), nseed,
                                     " ".join(float(v).hex() for v in w), run)


class _Cases:
    """The driver's input: every sector of C1, C2 and CN with the model's own
    seed table, a real and a complex random vector each; then the tables that
    must be refused, a few that must not, and the thermal factors."""

    def __init__(self, dirpath):
        from oracle.oracle import Oracle

        self.lines, self.expect = [], []
        rng = np.random.default_rng(5)
        for name in MODELS:
            cfg = ct.config(name)
            orc = Oracle(cfg)
            levels = chi.seed_levels(cfg)
            weights = [w for _, _, w in chi.seed_table(cfg)]
            self.lines.append(f"ns {cfg.Ns}")
            for s in ct.truth(name).secs:
                hmap = orc.build_sector(s.q1, s.q2)
                assert np.array_equal(hmap, ct.truth(name).maps[s.isector])
                self.lines.append("map %d %s" % (len(hmap), " ".join(str(int(m)) for m in hmap)))
                for cplx in (False, True):
                    x = rng.normal(size=len(hmap)) + (1j * rng.normal(size=len(hmap)) if cplx else 0.0)
                    flat = np.ascontiguousarray(x).view(np.float64)
                    self.lines.append("vec %d %s" % (int(cplx), " ".join(float(v).hex() for v in flat)))
                    self.lines.append(_table_line(levels, weights))
                    self.expect.append(("run", name, hmap, levels, weights, x))
        Ns = ct.config("C2").Ns                        # the last `ns` line: C2's and CN's differ
        self.lines.append(f"ns {Ns}")
        one = [[1.0]]
        bad = [
            ([], []),                                  # nlev = 0
            (list(range(7)), [[1.0] * 7]),             # nlev = 7
            ([0, 1, 0], [[1.0] * 3]),                  # duplicate level
            ([2 * Ns], one),                           # level = 2*Ns
            ([-1], one),                               # level < 0
            ([0], [[1.0]] * 33),                       # nseed = 33
        ]
        for lv, w in bad:
            self.lines.append(_table_line(lv, w, run=0))
            self.expect.append(("bad",))
        self.lines.append("table 1 0 0  0")            # nseed = 0
        self.expect.append(("bad",))
        good = [([2 * Ns - 1], one), ([0], [[0.5]] * 32), ([5, 4, 3, 2, 1, 0], [[1.0] * 6, [0.0] * 6])]
        for lv, w in good:
            self.lines.append(_table_line(lv, w, run=0))
            self.expect.append(("good",))
        for de in THERMAL_D:
            self.lines.append(f"thermal {float(ct.BETA).hex()} {float(de).hex()}")
            self.expect.append(("thermal", de))
        self.path = dirpath / "cases.txt"
        self.path.write_text("\n".join(self.lines) + "\n")


@pytest.fixture(scope="module")
def diag_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("seed_diag")
    c = _Cases(d)
    c.dir = d
    c.raw = subprocess.run([_build(d), str(c.path)], capture_output=True, text=True, check=True).stdout
    return c


def test_seed_diag_host_and_table_check(diag_run):
    c = diag_run
    rows = c.raw.strip().split("\n")
    assert len(rows) == len(c.expect)
    nrun = nbad = ngood = nth = nzero = 0
    worst = worst_n = 0.0
    for row, exp in zip(rows, c.expect):
        f = row.split()
        if exp[0] == "bad":
            assert f == ["1"], (row[:40], exp)            # ED_ERR_ARG
            nbad += 1
        elif exp[0] == "good":
            assert f == ["0"]
            ngood += 1
        elif exp[0] == "thermal":
            fh, sh = thermal_host(ct.BETA, exp[1])
            got_f, got_s = float.fromhex(f[0]), float.fromhex(f[1])
            assert abs(got_f - fh) <= 4e-16 * abs(fh) and abs(got_s - sh) <= 4e-16 * abs(sh), (exp, got_f, got_s)
            if exp[1] == 0.0:
                assert got_s == ct.BETA and got_f == 0.0
            nth += 1
        else:
            _, name, hmap, levels, weights, x = exp
            assert f[0] == "0"
            vals = np.array([float.fromhex(t) for t in f[1:]])
            n2, seeds = vals[:len(weights)], vals[len(weights):]
            seeds = (seeds.view(np.complex128) if np.iscomplexobj(x) else seeds).reshape(len(weights), len(hmap))
            ref = numpy_seeds(hmap, levels, weights, x)
            # one factor (the same additions in the same order) and one product per element: the same bits
            worst = max(worst, np.max(np.abs(seeds - ref)))
            for q in range(len(weights)):
                r2 = float(np.vdot(ref[q], ref[q]).real)
                if r2 == 0.0:
                    assert n2[q] == 0.0 and not np.any(seeds[q])
                    nzero += 1
                else:
                    worst_n = max(worst_n, abs(n2[q] - r2) / r2)
            nrun += 1
    print(f"{nrun} runs: max |host - numpy| {worst:.2e}, norm2 {worst_n:.2e}, {nzero} zero seeds; {nbad} tables refused, "
          f"{ngood} accepted, {nth} thermal factors")
    assert nrun == 2 * (16 + 25 + 7) and nbad == 7 and ngood == 3 and nth == len(THERMAL_D)
    assert nzero > 0                                   # e.g. Sz of the empty sector
    assert worst == 0.0 and worst_n < 1e-14


def test_driver_clean_under_sanitizers(diag_run):
    """The same driver and cases under AddressSanitizer + UBSan (host code with
    its own main): no report, same output."""
    exe = _build(diag_run.dir, ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe, str(diag_run.path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    assert out.stdout == diag_run.raw
