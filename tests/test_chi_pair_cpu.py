"""Pair and inter-orbital density susceptibilities (edgpu.chi.build_chi with
pair / exc; build_chi_pair ED_GF_CHIPAIR.f90 and lanc_ed_build_densChi_mix_c
ED_GF_CHIDENS.f90:490-673) on the CPU: the host half of
the two-operator seed kernel (csrc/ed_seed_pair.hpp) through a stand-alone C++
driver against forward-form numpy seeds, the component layout, and the whole
chain in numpy (chi_pair_host.replay_chi_pair) against the dense Lehmann sums
of chi_pair_truth.

Bars.  chi(iv) and chi(tau): 1e-10 of each array's maximum.  chi(w): the
project's 1e-5.  Measured with this file's replay (max over every pair row and
every off-diagonal exc entry of |replay - truth| / max|truth array|; Lmats =
32, Ltau = 24, Lreal = 32 on [-5, 5], beta = 8, T = 0 lists from the dense
ground states), chi(w):

    eps     C1         C2         CN         thermal C1
    0.01    7.8e-15    3.5e-14    1.4e-14    2.6e-14
    0.1     3.7e-15    6.0e-15    1.5e-15    1.3e-14
    0.2     2.1e-15    3.0e-15    6.2e-16    7.2e-15
    0.3     1.5e-15    1.8e-15    3.6e-16    5.2e-15
    0.5     1.1e-15    1.4e-15    2.1e-16    3.5e-15

Every model holds 1e-5 at the smallest listed eps, 0.01 (chi_pair_truth.EPS),
and the GPU test uses it.  On the other two grids the replay is within
4.7e-16 / 5.5e-16 (C1: iv / tau), 2.6e-15 / 1.0e-15 (C2, 3 degenerate
states), 1.6e-16 / 1.1e-16 (CN) and 3.6e-15 / 9.2e-16 (thermal C1, 7 states,
2 twin entries) of the truth.  The pair target sectors of the T = 0 lists
have no pole nearer than |D| = 0.77 (C2; C1 1.34, CN 1.46); the smallest
norm2 of a T = 0 pair or exc seed is 1.6e-5 (C2); the smallest share of a
compared array that comes from poles with |D| > 1e-6 is 0.66 (C2, exc).
"""
import os
import subprocess

import numpy as np
import pytest

import chi_pair_truth as pt
import chi_truth as ct
from chi_pair_host import chi_poles_host_signed, forward_image, numpy_pair_seeds, replay_chi_pair
from edgpu import chi
from edgpu.diag import DiagOptions, StateList, post_diag, state_list
from edgpu.params import MODES, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmft-ed_amd", "csrc")
MODELS = ["C1", "C2", "CN"]


def ground_list(name):
    T = ct.truth(name)
    return state_list(T.sector_results(2), DiagOptions(), T.cfg)


def thermal_list():
    T = ct.truth("C1")
    opt = DiagOptions(lanc_nstates_total=ct.NTOTAL, beta=ct.BETA, cutoff=ct.CUTOFF, ed_twin=True)
    sl, _ = post_diag(state_list(T.sector_results(6, True), opt, T.cfg), opt, T.cfg)
    return sl


# ------------------------------------------------------------ layout
def test_existing_layout_is_unchanged():
    """pair / exc left off: the helpers give the counts they gave before."""
    c1, c2, c3 = ct.config("C1"), ct.config("C2"), make_config(Norb=3, Nbath=1)
    assert [chi.n_components(c) for c in (c1, c2, c3)] == [4, 7, 11]
    assert [chi.n_components_ext(c) for c in (c1, c2, c3)] == [4, 7, 11]
    assert [len(chi.seed_table(c)) for c in (c1, c2, c3)] == [2, 7, 11]
    sl = StateList([0.0, 0.0], [9, 13], [None, None])
    assert len(chi.chi_jobs(c2, sl)) == 14
    assert chi.seed_pair_calls(c2) == [] and chi.seed_pair_calls(c1, exc=True) == []      # Norb = 1: no exc seed
    copt = chi.ChiOptions(Lmats=2, Ltau=3, Lreal=4, beta=2.0)
    iv, tau, w = np.ones((7, 3), complex), np.ones((7, 4)), np.ones((7, 4), complex)
    a, b = chi.assemble(c2, copt, iv, tau, w), chi.assemble_ext(c2, copt, iv, tau, w)
    for f in ("spin_iv", "spin_tau", "spin_w", "dens_iv", "dens_tau", "dens_w", "dens_tot_iv", "dens_tot_tau", "dens_tot_w"):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    for f in ("pair_iv", "pair_tau", "pair_w", "exc_iv", "exc_tau", "exc_w"):
        assert getattr(a, f) is None and getattr(b, f) is None


def test_new_components_sit_behind_the_existing_ones():
    cfg = make_config(Norb=3, Nbath=1)
    Ns = cfg.Ns
    assert chi.n_components_ext(cfg, pair=True) == 14 and chi.n_components_ext(cfg, exc=True) == 20
    assert chi.n_components_ext(cfg, True, True) == 23
    assert [chi.pair_component(cfg, a) for a in range(3)] == [11, 12, 13]
    assert chi.exc_component(cfg, 0, 1) == 12 and chi.exc_component(cfg, 2, 1, pair=True) == 14 + 7
    calls = chi.seed_pair_calls(cfg, True, True)
    assert [c[0] for c in calls] == [-1, +1, 0]
    assert calls[0][1] == [(a + Ns, 0, a, 0) for a in range(3)]       # c on (a, dw), then c on (a, up)
    assert calls[1][1] == [(a, 1, a + Ns, 1) for a in range(3)]       # c^+ on (a, up), then c^+ on (a, dw)
    assert calls[0][2] == [(0, -1), (1, -1), (2, -1)]
    assert [q for q in calls[0][3]] == [[(("pair", a), 11 + a, -1)] for a in range(3)]
    assert [q for q in calls[1][3]] == [[(("pair", a), 11 + a, +1)] for a in range(3)]
    _, images, terms, queue = calls[2]
    assert len(images) == 12 and len(terms) == 6                      # the limits of one call at ED_MAX_NORB
    assert chi.exc_pairs(cfg) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert images[:2] == [(0, 0, 1, 1), (Ns, 0, 1 + Ns, 1)] and terms[0] == (0, 1) and terms[5] == (10, 11)
    assert queue[0] == [(("exc", 0, 1), 14 + 1, +1), (("exc", 1, 0), 14 + 3, -1)]
    comps = sorted(c for q in queue for _, c, _ in q)
    assert comps == sorted(2 * [14 + 3 * a + b for a in range(3) for b in range(3) if a != b])
    # the assembled fields
    copt = chi.ChiOptions(Lmats=2, Ltau=3, Lreal=4, beta=2.0)
    val = np.arange(23.0)
    out = chi.assemble_ext(cfg, copt, val[:, None] * np.ones((23, 3), complex), val[:, None] * np.ones((23, 4)),
                           val[:, None] * np.ones((23, 4), complex), pair=True, exc=True)
    assert out.pair_iv.shape == (3, 3) and out.pair_tau.shape == (3, 4) and out.exc_w.shape == (3, 3, 4)
    assert np.array_equal(out.pair_tau[:, 0], [11, 12, 13]) and np.array_equal(out.exc_tau[:, :, 0], 14 + np.arange(9.0).reshape(3, 3))
    assert np.array_equal(out.spin_tau[:, 0], [0, 1, 2, 3])


def test_pair_target_sectors():
    from edgpu.sectors import get_sector

    cfg = ct.config("C2")
    by = get_sector(cfg)
    t = chi.pair_target(cfg, by[(2, 2)], -1)
    assert (t.q1, t.q2) == (1, 1) and (lambda u: (u.q1, u.q2))(chi.pair_target(cfg, by[(2, 2)], +1)) == (3, 3)
    assert chi.pair_target(cfg, by[(0, 2)], -1) is None and chi.pair_target(cfg, by[(2, 0)], -1) is None
    assert chi.pair_target(cfg, by[(cfg.Ns, 1)], +1) is None
    cn = ct.config("CN")
    byn = get_sector(cn)
    assert chi.pair_target(cn, byn[(3, 0)], +1).q1 == 5 and chi.pair_target(cn, byn[(3, 0)], -1).q1 == 1
    assert chi.pair_target(cn, byn[(1, 0)], -1) is None and chi.pair_target(cn, byn[(5, 0)], +1) is None


def test_refusals_name_the_part():
    jz = make_config(Norb=3, Nbath=1, Nspin=2, ed_mode="nonsu2", Jz_basis=True)
    sl = StateList([0.0], [1], [np.ones(1)])
    o = chi.ChiOptions(Lmats=4, Lreal=4, Ltau=4)
    with pytest.raises(NotImplementedError, match="pair"):
        chi.build_chi(jz, sl, o, pair=True)
    with pytest.raises(NotImplementedError, match="exc"):
        chi.build_chi(jz, sl, o, exc=True)
    sc = make_config(Norb=1, Nbath=2, ed_mode="superc", deltasc=0.3)
    with pytest.raises(NotImplementedError, match="superc"):
        chi.build_chi(sc, sl, o, pair=True, exc=True)


# ------------------------------------------------------------ the signed pole sum
def test_one_sign_fractions_add_up_to_the_two_sign_one():
    """A +1 and a -1 fraction of the same poles are the two halves of a both-sign one."""
    from chi_host import chi_poles_host

    beta, eps = 8.0, 0.05
    vm, tg, wr = chi.bosonic_matsubara(beta, 3), chi.tau_grid(beta, 4), np.array([-1.0, 0.2])
    E, z = [-1.0 + 0.3, -1.0 - 0.2, -1.0], [0.6, 0.5, 0.3]
    both = chi_poles_host_signed([(0, 0.5, -1.0, E, z, 0)], beta, vm, tg, wr, eps, 1)
    old = chi_poles_host([(0, 0.5, -1.0, E, z)], beta, vm, tg, wr, eps, 1)
    for a, b in zip(both[:3], old[:3]):
        assert np.array_equal(a, b)                        # isign = 0: the arithmetic of chi_poles_host, bit for bit
    plus = chi_poles_host_signed([(0, 0.5, -1.0, E, z, +1)], beta, vm, tg, wr, eps, 1)
    two = chi_poles_host_signed([(0, 0.5, -1.0, E, z, +1), (0, 0.5, -1.0, E, z, -1)], beta, vm, tg, wr, eps, 1)
    for a, b in zip(two[:3], both[:3]):
        assert np.array_equal(a, b)                        # the same additions in the same order
    # one pole by hand, +1 alone
    D, p = 0.3, 0.5 * 0.36
    one = chi_poles_host_signed([(0, 0.5, -1.0, [-1.0 + D], [0.6], +1)], beta, vm, tg, wr, eps, 1)
    f = 1.0 - np.exp(-beta * D)
    assert abs(one[0][0, 0] - p * f / D) < 1e-14
    np.testing.assert_allclose(one[0][0, 1:], -p * f / (1j * vm[1:] - D), rtol=1e-14)
    np.testing.assert_allclose(one[1][0], p * np.exp(-tg * D), rtol=1e-14)
    np.testing.assert_allclose(one[2][0], -p * f / (wr + 1j * eps - D), rtol=1e-14)
    minus = chi_poles_host_signed([(0, 0.5, -1.0, [-1.0 + D], [0.6], -1)], beta, vm, tg, wr, eps, 1)
    np.testing.assert_allclose(minus[1][0], p * np.exp(-(beta - tg) * D), rtol=1e-14)
    np.testing.assert_allclose(minus[2][0], p * f / (wr + 1j * eps + D), rtol=1e-14)
    assert np.any(plus[1] != both[1])


# ------------------------------------------------------------ the chain against the dense truth
@pytest.mark.parametrize("name", MODELS)
def test_replay_matches_the_dense_truth(name):
    T, copt, sl = pt.truth(name), pt.options(name), ground_list(name)
    cfg, No = T.cfg, T.cfg.Norb
    rec = []
    got = replay_chi_pair(cfg, sl, copt, record=rec)
    d = pt.distances(T.pair_exc_of_list(sl, copt), got, No)
    print(f"{name}: {sl.size} state(s) in sectors {sl.sectors}, eps {copt.eps}: iv {d[0]:.2e}, tau {d[1]:.2e}, "
          f"w {d[2]:.2e}; smallest dynamic share {min(T.shares.values()):.2e}, smallest |D| of a pair pole "
          f"{T.min_abs_d_pair:.3f}, smallest norm2 {T.min_amp2:.2e}")
    assert T.min_abs_d_pair > 1e-6 and T.min_amp2 > 0.0
    # queue order: kept state, pair -1 by orbital, pair +1, then every exc seed with +1 and -1; no seed vanished
    per_state = ([(("pair", a), -1) for a in range(No)] + [(("pair", a), +1) for a in range(No)]
                 + [x for a, b in chi.exc_pairs(cfg) for x in ((("exc", a, b), +1), (("exc", b, a), -1))])
    assert [(r["state"], r["name"], r["isign"]) for r in rec] == [(k,) + x for k in range(sl.size) for x in per_state]
    assert got.pair_iv.shape == (No, ct.LMATS + 1) and got.pair_tau.shape == (No, ct.LTAU + 1)
    assert got.exc_w.shape == (No, No, ct.LREAL) and got.spin_iv is None and got.dens_w is None
    for a in range(No):
        assert not np.any(got.exc_iv[a, a]) and not np.any(got.exc_tau[a, a]) and not np.any(got.exc_w[a, a])
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5
    # exc_tau[a,b](tau) = exc_tau[b,a](beta - tau)
    for a, b in chi.exc_pairs(cfg):
        assert np.max(np.abs(got.exc_tau[a, b] - got.exc_tau[b, a][::-1])) <= 1e-12 * np.max(np.abs(got.exc_tau[a, b]))
    # a part left out leaves the other as it is
    p_only, e_only = replay_chi_pair(cfg, sl, copt, exc=False), replay_chi_pair(cfg, sl, copt, pair=False)
    assert p_only.exc_iv is None and e_only.pair_w is None
    for a, b in ((p_only.pair_iv, got.pair_iv), (p_only.pair_tau, got.pair_tau), (p_only.pair_w, got.pair_w),
                 (e_only.exc_iv, got.exc_iv), (e_only.exc_tau, got.exc_tau), (e_only.exc_w, got.exc_w)):
        assert np.array_equal(a, b)


def test_replay_of_the_thermal_list_with_twin_entries():
    T, copt, sl = pt.truth("C1"), pt.options("C1"), thermal_list()
    kept = T.thermal_states()
    assert sl.finite_t and sl.size == len(kept) and sum(p is not None for p in sl.twin_of) >= 1
    assert any(e > sl.emin + 0.05 for e in sl.energies)   # excited states: poles with D < 0
    got = replay_chi_pair(T.cfg, sl, copt)
    d = pt.distances(T.pair_exc_thermal(copt), got, 1)
    print(f"thermal C1: {sl.size} states, {sum(p is not None for p in sl.twin_of)} twin entries: iv {d[0]:.2e}, "
          f"tau {d[1]:.2e}, w {d[2]:.2e}")
    assert d[0] < 1e-10 and d[1] < 1e-10 and d[2] < 1e-5


# ------------------------------------------------------------ the plan header on the host
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ed_seed_pair.hpp"
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
    } else if (c == "plan") {   // nimg (lev1 op1 lev2 op2)... nseed (p q)... run
      const int nimg = (int)I();
      std::vector<int32_t> img(4 * std::max(nimg, 1));
      for (int l = 0; l < 4 * nimg; l++) img[l] = (int32_t)I();
      const int nseed = (int)I();
      std::vector<int32_t> terms(2 * std::max(nseed, 1));
      for (int s = 0; s < 2 * nseed; s++) terms[s] = (int32_t)I();
      const int run = (int)I();
      PairPlan P;
      const int rc = seed_pair_compile(S, nimg, img.data(), nseed, terms.data(), &P);
      printf("%d", rc);
      if (rc == ED_OK && run) {
        const size_t w = vc ? 2 : 1, dim = mdst.size();
        std::vector<double> seeds((size_t)nseed * dim * w), n2(nseed);
        seed_pair_host(P, (int64_t)dim, mdst.data(), x.data(), vc != 0,
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
    src = dirpath / "seed_pair_driver.cpp"
    src.write_text(DRIVER)
    exe = dirpath / ("seed_pair_driver" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", *extra, "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    return str(exe)


def _plan_line(images, terms, run=1):
    flat_i = [v for im in images for v in im]
    flat_t = [v for pq in terms for v in pq]
    return "plan %d %s %d %s %d" % (len(images), " ".join(map(str, flat_i)), len(terms), " ".join(map(str, flat_t)), run)


def c2_tables(Ns):
    """(dst, images, terms) of the normal-mode Norb = 2 model from the (2, 2) sector."""
    down = [(a + Ns, 0, a, 0) for a in range(2)] + [(Ns + 2, 0, 3, 0), (1, 0, Ns, 0)]        # lev2 < lev1 and lev2 > lev1
    up = [(a, 1, a + Ns, 1) for a in range(2)] + [(Ns + 3, 1, 2, 1)]
    exc = [(0, 0, 1, 1), (Ns, 0, Ns + 1, 1), (1, 0, 0, 1), (Ns + 1, 0, Ns, 1), (3, 0, 0, 1), (Ns, 1, Ns + 2, 0)]
    return [((1, 1), down, [(0, -1), (1, -1), (2, 3), (3, 0)]),
            ((3, 3), up, [(0, -1), (1, -1), (2, 1)]),
            ((2, 2), exc, [(0, 1), (2, 3), (4, -1), (5, 4), (0, 2)])]


def cn_tables(Ns):
    """The nonsu2 Norb = 1 model from N = 3: any two levels change N by two."""
    return [((5, 0), [(0, 1, Ns, 1), (1, 1, 2, 1), (Ns + 2, 1, 0, 1)], [(0, -1), (1, 2), (2, -1)]),
            ((1, 0), [(Ns, 0, 0, 0), (2, 0, 1, 0), (0, 0, Ns + 1, 0)], [(0, -1), (1, 2), (2, 0)]),
            ((3, 0), [(0, 0, Ns, 1), (Ns, 0, 0, 1), (1, 1, Ns + 2, 0)], [(0, 1), (2, -1)])]


class _Cases:
    """The driver's input: C2 from (2, 2) and CN from N = 3 into the pair and
    the own sectors, a real and a complex random vector each; then the plans
    that must be refused and a few that must not."""

    def __init__(self, dirpath):
        from oracle.oracle import Oracle

        self.lines, self.expect = [], []
        rng = np.random.default_rng(13)
        for name, src_q, tables in (("C2", (2, 2), c2_tables), ("CN", (3, 0), cn_tables)):
            cfg = ct.config(name)
            orc = Oracle(cfg)
            src = orc.build_sector(*src_q)
            for dst_q, images, terms in tables(cfg.Ns):
                dst = orc.build_sector(*dst_q)
                self.lines.append(f"sectors {cfg.Ns} {MODES[cfg.ed_mode]} {src_q[0]} {src_q[1]} {dst_q[0]} {dst_q[1]}")
                self.lines.append("maps %d %s %d %s" % (len(src), " ".join(str(int(m)) for m in src), len(dst),
                                                        " ".join(str(int(m)) for m in dst)))
                for cplx in (False, True):
                    x = rng.normal(size=len(src)) + (1j * rng.normal(size=len(src)) if cplx else 0.0)
                    flat = np.ascontiguousarray(x).view(np.float64)
                    self.lines.append("vec %d %s" % (int(cplx), " ".join(float(v).hex() for v in flat)))
                    self.lines.append(_plan_line(images, terms))
                    self.expect.append(("run", src, dst, images, terms, x))
        Ns = ct.config("C2").Ns
        self.lines.append(f"sectors {Ns} {MODES['normal']} 2 2 1 1")
        ok = [(Ns, 0, 0, 0), (Ns + 1, 0, 1, 0)]
        thirteen = [(Ns + j, 0, i, 0) for i in range(4) for j in range(4)][:13]
        bad = [
            ([(0, 0, 0, 0)], [(0, -1)]),                      # lev1 == lev2
            ([(0, 1, Ns, 1)], [(0, -1)]),                     # reaches (3, 3), not dst
            ([(0, 0, 1, 0)], [(0, -1)]),                      # two up electrons fewer: (0, 2)
            ([(0, 0, 1, 1)], [(0, -1)]),                      # stays in src
            (ok + [ok[0]], [(0, 1)]),                         # duplicate image
            (ok, [(1, 1)]),                                   # p == q
            (ok, [(0, 2)]),                                   # q >= nimg
            (ok, [(2, -1)]),                                  # p >= nimg
            (ok, [(-1, 0)]),                                  # p < 0
            ([(2 * Ns, 0, 0, 0)], [(0, -1)]),                 # level >= 2*Ns
            ([(Ns, 2, 0, 0)], [(0, -1)]),                     # op outside {0, 1}
            ([], [(0, -1)]),                                  # nimg = 0
            (thirteen, [(0, -1)]),                            # nimg = 13
            (ok, []),                                         # nseed = 0
            (ok, [(0, -1)] * 13),                             # nseed = 13
        ]
        for im, tt in bad:
            self.lines.append(_plan_line(im, tt, run=0))
            self.expect.append(("bad",))
        good = [(ok, [(0, 1)]), ([ok[1]], [(0, -1)]), (thirteen[:12], [(k, (k + 1) % 12) for k in range(12)]),
                ([(0, 0, Ns, 0)], [(0, -1)])]                 # the other order of the same two operators
        for im, tt in good:
            self.lines.append(_plan_line(im, tt, run=0))
            self.expect.append(("good",))
        self.path = dirpath / "cases.txt"
        self.path.write_text("\n".join(self.lines) + "\n")


@pytest.fixture(scope="module")
def pair_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("seed_pair")
    c = _Cases(d)
    c.dir = d
    c.raw = subprocess.run([_build(d), str(c.path)], capture_output=True, text=True, check=True).stdout
    return c


def test_plan_validation_and_row_rule_on_the_host(pair_run):
    c = pair_run
    rows = c.raw.strip().split("\n")
    assert len(rows) == len(c.expect)
    nrun = nbad = ngood = nzero = 0
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
            _, src, dst, images, terms, x = exp
            assert f[0] == "0"
            vals = np.array([float.fromhex(t) for t in f[1:]])
            n2, seeds = vals[:len(terms)], vals[len(terms):]
            seeds = (seeds.view(np.complex128) if np.iscomplexobj(x) else seeds).reshape(len(terms), len(dst))
            ref = numpy_pair_seeds(src, dst, images, terms, x)
            # one exact sign product, one product and at most one addition per element: the same bits
            worst = max(worst, np.max(np.abs(seeds - ref)))
            for s in range(len(terms)):
                r2 = float(np.vdot(ref[s], ref[s]).real)
                assert r2 > 0.0
                worst_n = max(worst_n, abs(n2[s] - r2) / r2)
            nzero += int(np.sum(ref == 0))
            nrun += 1
    print(f"{nrun} runs: max |host - numpy| {worst:.2e}, norm2 {worst_n:.2e}; {nbad} plans refused, {ngood} accepted")
    assert nrun == 12 and nbad == 15 and ngood == 4 and nzero > 0
    assert worst == 0.0 and worst_n < 1e-14


def test_forward_form_signs_by_hand():
    """The forward form on the one state |0b011> against signs worked out by hand."""
    src = np.array([0b011], dtype=np.uint32)
    # c_0 |011> = +|010>; c^+_2 |010> = -|110> (one electron below level 2)
    assert list(forward_image(src, np.array([0b110], dtype=np.uint32), (0, 0, 2, 1), np.array([1.0]))) == [-1.0]
    # c_1 |011> = -|001>; c_0 |001> = +|000>
    assert list(forward_image(src, np.array([0b000], dtype=np.uint32), (1, 0, 0, 0), np.array([1.0]))) == [-1.0]
    # c_0 |011> = +|010>; c_1 |010> = +|000>
    assert list(forward_image(src, np.array([0b000], dtype=np.uint32), (0, 0, 1, 0), np.array([1.0]))) == [1.0]
    # c^+_0 on an occupied level: nothing
    assert list(forward_image(src, np.array([0b111], dtype=np.uint32), (0, 1, 2, 1), np.array([1.0]))) == [0.0]


def test_driver_clean_under_sanitizers(pair_run):
    """The same driver and cases under AddressSanitizer + UBSan (host code with
    its own main): no report, same output."""
    exe = _build(pair_run.dir, ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe, str(pair_run.path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    assert out.stdout == pair_run.raw
