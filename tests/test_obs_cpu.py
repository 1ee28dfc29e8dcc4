"""The host half of the observables (dmft-ed_amd/csrc/ed_obs.hpp) and
edgpu.observables on the CPU: no GPU, no HIP.

A stand-alone C++ driver (its own main, compiled here with plain g++)
compiles operator strings for a sector and evaluates them with the serial
host evaluator — the same obs_row the kernel calls — on a map and a vector
read from a file; results are printed as hex floats.  The truth is built from
the full-Fock Jordan-Wigner matrices of oracle.jw_dense._ops multiplied in
string order (obs_truth.dense_expect).  Vectors are random, complex and of
unit norm: eigenvectors would hide sign errors behind their symmetry.

Tolerance 1e-12 absolute: for a unit vector sum_i |conj(v_j) v_i| <= 1, so two
double-precision summation orders differ by at most about dim*eps = 792 *
2.2e-16 < 2e-13 at the largest sector used here.

edgpu.observables / local_energy run through their `evaluator` hook with
obs_truth's numpy walk, against the dense eigh of every sector traced over
the degenerate ground multiplet; the same on two gloo ranks with split owners.
"""
import os
import socket
import subprocess

import numpy as np
import pytest

import cases
import obs_truth as ot
from edgpu.params import MODES, make_config
from edgpu.sectors import LZDIAG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmft-ed_amd", "csrc")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ed_obs.hpp"
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
  ObsSector S{0, 0, 0, nullptr};
  std::vector<int32_t> lz2;
  std::vector<uint32_t> map;
  std::vector<double> v;
  int vc = 0;
  for (std::string c = tok(); !c.empty(); c = tok()) {
    if (c == "sector") {
      S.ns = (int)I(); S.mode = (int)I(); S.jz = (int)I();
      lz2.resize(S.ns);
      for (auto& x : lz2) x = (int32_t)I();
      S.lz2 = lz2.data();
    } else if (c == "vec") {
      const long dim = I();
      vc = (int)I();
      map.resize(dim);
      for (auto& m : map) m = (uint32_t)I();
      v.resize((size_t)dim * (vc ? 2 : 1));
      for (auto& x : v) x = D();
    } else if (c == "term") {
      const int nop = (int)I();
      std::vector<int32_t> lev(std::max(nop, 1)), op(std::max(nop, 1));
      for (int k = 0; k < nop; k++) lev[k] = (int32_t)I();
      for (int k = 0; k < nop; k++) op[k] = (int32_t)I();
      ObsTerm t;
      const int rc = obs_compile(S, nop, lev.data(), op.data(), &t);
      double re = 0.0, im = 0.0;
      if (rc == ED_OK)
        obs_expect_host(t, (int64_t)map.size(), map.data(), v.data(), vc != 0,
                        [&](uint32_t k) { return (int64_t)(std::lower_bound(map.begin(), map.end(), k) - map.begin()); },
                        &re, &im);
      printf("%d %a %a\n", rc, re, im);
    } else {
      return 3;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("obs")
    src = d / "obs_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "obs_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    return str(exe), d


def run_driver(driver, cfg, hmap, vec, terms, tag):
    exe, d = driver
    Ns = cfg.Ns
    lz2 = [2 * LZDIAG[l % cfg.Norb] for l in range(Ns)]
    cplx = np.iscomplexobj(vec)
    flat = np.ascontiguousarray(vec).view(np.float64)
    lines = ["sector %d %d %d %s" % (Ns, MODES[cfg.ed_mode], int(cfg.Jz_basis), " ".join(map(str, lz2))),
             "vec %d %d %s %s" % (len(hmap), int(cplx), " ".join(str(int(m)) for m in hmap),
                                  " ".join(float(x).hex() for x in flat))]
    for t in terms:
        lines.append("term %d %s %s" % (len(t), " ".join(str(l) for l, _ in t), " ".join(str(o) for _, o in t)))
    path = d / f"{tag}.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    res = []
    for ln in out[: len(terms)]:
        rc, re, im = ln.split()
        res.append((int(rc), complex(float.fromhex(re), float.fromhex(im))))
    assert len(res) == len(terms)
    return res


CASES = {c[0]: c[1] for c in cases.CASES}
SECTORS = [("normal_jh", (3, 3)), ("nonsu2_rand", (5, 0)), ("superc_2orb", (1, 0)), ("nonsu2_jz", (5, 1))]


def case_terms(cfg):
    terms = ot.hop_terms(cfg) + ot.number_terms(cfg)
    if cfg.Norb > 1:
        terms += ot.exchange_terms(cfg)
    terms += ot.pair_terms(cfg)     # conserving only in superc
    return terms


@pytest.mark.parametrize("name,q", SECTORS)
def test_host_terms_match_dense_operators(driver, name, q):
    from oracle.oracle import Oracle

    cfg = CASES[name]()
    hmap = Oracle(cfg).build_sector(*q)
    vec = ot.random_state(len(hmap), True, seed=len(hmap))
    terms = case_terms(cfg)
    res = run_driver(driver, cfg, hmap, vec, terms, name)
    nlev = 2 * cfg.Ns
    naccept = nreject = 0
    worst = 0.0
    for t, (rc, val) in zip(terms, res):
        vanishes = ot.dense_term(nlev, t).nnz == 0
        if vanishes or ot.dense_conserves(cfg, t):
            assert rc == 0, (t, rc)
            worst = max(worst, abs(val - ot.dense_expect(nlev, hmap, vec, t)))
            naccept += 1
        else:
            assert rc == 1, (t, rc)         # ED_ERR_ARG
            nreject += 1
    print(f"{name} {q}: dim {len(hmap)}, {naccept} strings, max |host - dense| = {worst:.3e}, {nreject} rejected")
    assert worst < 1e-12
    assert naccept >= 2 * 2 * cfg.Norb + 3 and nreject >= 1
    # the number operator both ways round: <c_p c+_p> = 1 - <c+_p c_p> on a unit vector
    k = len(ot.hop_terms(cfg))
    nl = 2 * cfg.Norb
    for p in range(nl):
        assert abs(res[k + p][1] + res[k + nl + p][1] - 1.0) < 1e-12


def test_real_vector_gives_real_values(driver):
    from oracle.oracle import Oracle

    cfg = CASES["normal_jh"]()
    hmap = Oracle(cfg).build_sector(3, 3)
    vec = ot.random_state(len(hmap), False, seed=5)
    terms = [t for t in case_terms(cfg) if ot.dense_term(2 * cfg.Ns, t).nnz and ot.dense_conserves(cfg, t)]
    for t, (rc, val) in zip(terms, run_driver(driver, cfg, hmap, vec, terms, "real")):
        assert rc == 0 and val.imag == 0.0
        assert abs(val - ot.dense_expect(2 * cfg.Ns, hmap, vec.astype(np.complex128), t)) < 1e-12


def test_rejected_strings(driver):
    """Every string that does not map the sector into itself, or is malformed,
    is refused by the compile step (ED_ERR_ARG = 1)."""
    from oracle.oracle import Oracle

    def rcs(name, q, terms):
        cfg = CASES[name]()
        hmap = Oracle(cfg).build_sector(*q)
        return cfg, [rc for rc, _ in run_driver(driver, cfg, hmap, ot.random_state(len(hmap), True, 1), terms,
                                                "rej_" + name)]

    cfg = CASES["normal_jh"]()
    Ns = cfg.Ns
    bad = [[(0, 1), (Ns, 0)],                 # spin flip in normal mode
           [(0, 1), (1, 1)],                  # c+ c+
           [(0, 0)],                          # a single annihilator
           [],                                # no operator
           [(0, 1), (0, 0)] * 2 + [(1, 1)],   # five operators
           [(2 * Ns, 1), (2 * Ns, 0)],        # level >= 2*Ns
           [(-1, 1), (-1, 0)],
           [(0, 2), (0, 0)]]                  # op outside {0, 1}
    assert rcs("normal_jh", (3, 3), bad)[1] == [1] * len(bad)
    cfg = CASES["superc_2orb"]()
    Ns = cfg.Ns
    _, r = rcs("superc_2orb", (1, 0), [[(0, 1), (Ns, 0)], [(0, 0), (1, 0)], [(0, 0), (Ns, 0)], [(0, 1), (Ns, 1)]])
    assert r == [1, 1, 0, 0]                  # spin flip, c_up c_up refused; the pair operators keep sz
    cfg = CASES["nonsu2_jz"]()
    Ns = cfg.Ns
    _, r = rcs("nonsu2_jz", (5, 1), [[(0, 1), (1, 0)],          # Lz -1 <- +1: changes Jz
                                     [(0, 1), (Ns, 0)],         # same orbital spin flip: changes Jz
                                     [(0, 1), (0, 0)],
                                     [(1, 0), (1, 1)]])
    assert r == [1, 1, 0, 0]
    _, r = rcs("nonsu2_rand", (5, 0), [[(0, 1), (cfg.Ns, 0)], [(0, 1)], [(0, 1), (1, 1), (2, 0)]])
    assert r[1:] == [1, 1]


def test_numpy_walk_matches_dense():
    """The vectorised numpy walk (the evaluator of the tests below and the host
    route of the timing) agrees with the dense operators."""
    from oracle.oracle import Oracle

    for name, q in SECTORS:
        cfg = CASES[name]()
        hmap = Oracle(cfg).build_sector(*q)
        vec = ot.random_state(len(hmap), True, seed=3)
        for t in case_terms(cfg):
            if ot.dense_term(2 * cfg.Ns, t).nnz and ot.dense_conserves(cfg, t):
                assert abs(ot.numpy_expect(hmap, vec, t) - ot.dense_expect(2 * cfg.Ns, hmap, vec, t)) < 1e-12
        lv = ot.imp_levels(cfg)
        M, norm = ot.numpy_moments(hmap, vec, lv)
        assert abs(norm - 1.0) < 1e-12
        for a, p in enumerate(lv):
            for b, r in enumerate(lv):
                nn = [(p, 1), (p, 0), (r, 1), (r, 0)]
                assert abs(M[a, b] - ot.dense_expect(2 * cfg.Ns, hmap, vec, nn)) < 1e-12


def small_configs():
    rng = np.random.default_rng(4)
    h2 = np.zeros((2, 2, 1, 1), dtype=np.complex128)
    h2[0, 0, 0, 0], h2[1, 1, 0, 0] = 0.15, -0.1
    h2[0, 1, 0, 0], h2[1, 0, 0, 0] = 0.2 + 0.1j, 0.2 - 0.1j
    a = rng.normal(size=(2, 2))
    hj = np.zeros((1, 1, 2, 2), dtype=np.complex128)
    hj[0, 0] = 0.2 * (a + a.T)
    return {
        "normal": dict(Norb=1, Nbath=2),     # three sites at half filling: a spin doublet in (2,1) and (1,2)
        "normal_doped": dict(Norb=1, Nbath=2, xmu=0.7, bath="random", seed=3),
        "nonsu2": dict(Norb=1, Nbath=2, Nspin=2, ed_mode="nonsu2", bath="random", seed=5, xmu=0.3, impHloc=h2),
        "superc": dict(Norb=1, Nbath=2, ed_mode="superc", deltasc=0.3, bath="random", seed=6, xmu=0.2),
        "normal_2orb": dict(Norb=2, Nbath=1, Uloc=(2.0, 1.6, 0.0), Ust=1.0, Jh=0.3, Jx=0.3, Jp=0.2, xmu=0.4,
                            bath="random", seed=8, impHloc=hj),
    }


@pytest.mark.parametrize("name", list(small_configs()))
def test_observables_and_energy_match_dense_eigh(name):
    from edgpu.observables import local_energy, observables

    cfg = make_config(**small_configs()[name])
    states = ot.dense_ground_states(cfg)
    truth = ot.dense_observables(cfg, states)
    ev = ot.numpy_evaluator(ot.oracle_map)
    obs = observables(cfg, states, evaluator=ev)
    ene = local_energy(cfg, states, evaluator=ev)
    dev = ot.max_deviation(obs, ene, truth)
    print(f"{name}: {states.size} kept state(s), dens {obs.dens}, epot {ene.epot:.12f}, max deviation {dev:.3e}")
    assert dev < 1e-12
    assert abs(obs.s2tot - np.sum(obs.sz2)) < 1e-14


def test_weights_are_the_callers():
    from edgpu.observables import observables

    cfg = make_config(**small_configs()["normal"])
    states = ot.dense_ground_states(cfg)
    ev = ot.numpy_evaluator(ot.oracle_map)
    one = observables(cfg, states, evaluator=ev)
    two = observables(cfg, states, evaluator=ev, weights=[2.0 / states.size] * states.size)
    np.testing.assert_allclose(two.dens, 2.0 * one.dens, rtol=0, atol=1e-14)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, q, cfg_kw):
    import torch.distributed as dist

    from edgpu.diag import StateList
    from edgpu.observables import local_energy, observables

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = make_config(**cfg_kw)
    states = ot.dense_ground_states(cfg)
    owners = [k % world for k in range(states.size)]
    held = StateList(list(states.energies), list(states.sectors),
                     [v if owners[k] == rank else None for k, v in enumerate(states.vectors)])
    ev = ot.numpy_evaluator(ot.oracle_map)
    obs = observables(cfg, held, owners=owners, evaluator=ev)
    ene = local_energy(cfg, held, owners=owners, evaluator=ev)
    q.put((rank, obs, ene))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_two_ranks_match_one():
    """Split owners over 2 gloo ranks (each rank holds only its own vectors),
    one all_reduce: equal to the 1-rank result to 1e-13 on every rank."""
    import torch.multiprocessing as mp
    from dataclasses import asdict

    from edgpu.observables import local_energy, observables

    kw = small_configs()["normal"]
    cfg = make_config(**kw)
    states = ot.dense_ground_states(cfg)
    assert states.size >= 2          # a multiplet to split
    ev = ot.numpy_evaluator(ot.oracle_map)
    obs0, ene0 = observables(cfg, states, evaluator=ev), local_energy(cfg, states, evaluator=ev)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, kw)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(o[0] for o in out) == [0, 1]
    for _, obs, ene in out:
        for ref, got in ((asdict(obs0), asdict(obs)), (asdict(ene0), asdict(ene))):
            for k, v in ref.items():
                if v is not None:
                    assert np.max(np.abs(np.asarray(got[k]) - np.asarray(v))) < 1e-13, k
