"""Orbital off-diagonal Green's function of hybrid / replica baths
(lanc_build_gf_normal_mix_c, ED_GF_NORMAL.f90:279-553) on the CPU: the pair
list, the job list, and build_gf through the oracle job runner against the
dense direct Lehmann sum of orbmix_truth.

Bars.  G(iw): 1e-10 of max|G|, the project's bar.  G(w): 1e-8 of max|G| at a
broadening at which the continued fraction is not dominated by round-off.
The seeds go through the reference's plain Lanczos without
reorthogonalisation for nlanc = min(dim, 200) steps, which in these small
sectors is the whole dimension; poles that far into the loss of orthogonality
move with the last bits of the seed, and a broadening eps weighs that by
1/eps^2.  Measured with the oracle pipeline (oracle_gf_orbmix, every element
of every normalised seed multiplied by 1 + 1e-15 N(0,1), worst of 8 draws,
max over all components of |dG(w)| / max|G(w)|; Lreal = 32 on [-5, 5]), and
beside it the distance of the unperturbed pipeline from the dense truth:

    eps    H2 moved   H2 truth   H3 moved   H3 truth   RC moved   RC truth
    0.1    1.5e-09    4.9e-10    3.3e-06    7.4e-06    2.1e-08    7.8e-09
    0.2    6.6e-14    8.5e-14    8.8e-09    6.6e-08    5.0e-12    1.8e-12
    0.3    3.7e-14    5.8e-14    9.4e-11    6.9e-10    1.5e-13    6.1e-14
    0.5    1.7e-14    3.4e-14    2.3e-14    1.3e-13    7.7e-14    2.3e-14

At eps = 0.1 every model moves by more than 1e-9, so each is checked at the
smallest listed eps at which it does not (orbmix_truth.EPS: H2 0.2, H3 0.3,
RC 0.2); the 1e-8 bar stays.  On the Matsubara axis the same pipeline is
within 1.7e-13 of the truth for all three.
"""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import cases
import orbmix_truth as ot
from edgpu.diag import DiagOptions
from edgpu.farm import farm_diag
from edgpu.gf import GFOptions, _job_list, build_gf, matsubara, orbital_pairs, realaxis
from edgpu.params import make_config
from edgpu.sectors import c_sector, cdg_sector, setup_pointers

MODELS = ["H2", "H3", "RC"]
_RUN = {}


def gopt(name, **kw):
    return GFOptions(Lmats=32, Lreal=32, eps=ot.EPS[name], **kw)


def run(name):
    """farm_diag with the oracle solver + build_gf with the oracle job runner, once per model."""
    if name not in _RUN:
        from oracle_gf import oracle_job_runner
        from oracle_solver import solve_sector_oracle

        cfg = ot.truth(name).cfg
        sl = farm_diag(cfg, DiagOptions(lanc_method="lanczos"), solver=solve_sector_oracle).states
        Gm, Gr = build_gf(cfg, sl, gopt(name), runner=oracle_job_runner)
        _RUN[name] = dict(sl=sl, Gm=Gm, Gr=Gr)
    return _RUN[name]


def test_orbital_pairs():
    assert orbital_pairs(ot.config("H3")) == [(0, 0, 1), (0, 0, 2), (0, 1, 2), (1, 0, 1), (1, 0, 2), (1, 1, 2)]
    assert orbital_pairs(cases.normal_3orb()) == []
    assert orbital_pairs(cases.replica_cplx()) == [(0, 0, 1)]
    cfg = cases.replica_cplx()
    cfg.impHloc = cases._hloc(1, 2, 8, cplx=True, offdiag=False)
    assert orbital_pairs(cfg) == []
    assert orbital_pairs(cases.nonsu2_rand()) == [] and orbital_pairs(cases.superc_2orb()) == []


def test_job_list_orders_mixed_jobs_after_the_diagonal():
    cfg = ot.config("H3")
    sl = run("H3")["sl"]
    jobs, _ = _job_list(cfg, sl)
    tags = [j[1][0] for j in jobs]
    nd = tags.index("orbmix")
    assert set(tags[:nd]) == {"diag"} and set(tags[nd:]) == {"orbmix"}
    assert [j[0] for j in jobs[:nd]] == [j[0] for j in _job_list(cfg, sl, orbital_mix=False)[0]]
    Ns, secs = cfg.Ns, setup_pointers(cfg)
    at = nd
    for s, a, b in orbital_pairs(cfg):                       # the reference's loop order
        i, j = a + s * Ns, b + s * Ns
        want = [(1, +1, s, [(i, 1), (j, 1)], 1.0), (0, -1, s, [(i, 1), (j, 1)], 1.0),
                (1, +1, s, [(i, 1), (j, 1j)], -1j), (0, -1, s, [(i, 1), (j, -1j)], -1j)]
        for k, isec in enumerate(sl.sectors):
            sec = secs[isec - 1]
            for spec in want:
                tgt = cdg_sector(cfg, sec, s) if spec[0] == 1 else c_sector(cfg, sec, s)
                if tgt is None:
                    continue
                comp, tag, kk, got, src, dst = jobs[at]
                assert comp == (s, s, a, b) and tag == ("orbmix", s, a, b) and kk == k
                assert got == spec and src.isector == isec and dst.isector == tgt.isector
                at += 1
    assert at == len(jobs) and at - nd == 6 * 4 * sl.size    # (1,3): all four targets exist


def test_jobs_have_names_and_still_unpack():
    """`_job_list(...)[0][0]`: six fields by position and by name, the seed five."""
    jobs, _ = _job_list(ot.config("H3"), run("H3")["sl"])
    job = jobs[0]
    comp, tag, k, seed, src, dst = job
    assert len(job) == 6 and (job.comp, job.tag, job.k, job.seed, job.src, job.dst) == (comp, tag, k, seed, src, dst)
    assert job.seed.terms is job[3][3] and job.dst is job[5] and job.src is job[4]
    op, isign, ispin, terms, weight = seed
    assert (seed.op, seed.isign, seed.ispin, seed.terms, seed.weight) == (op, isign, ispin, terms, weight)
    assert seed == (1, +1, 0, [(0, 1)], 1.0) and job[:3] == ((0, 0, 0, 0), ("diag", 0, 0), 0)


@pytest.mark.parametrize("name", MODELS)
def test_offdiagonal_g_matches_the_dense_lehmann_sum(name):
    T, r = ot.truth(name), run(name)
    cfg, g = T.cfg, gopt(name)
    if name == "H2":
        assert r["sl"].size == 2          # the twin pair, both kept
    Tm, Tr = T.gf(matsubara(g.beta, g.Lmats), realaxis(g.wini, g.wfin, g.Lreal), g.eps)
    P = orbital_pairs(cfg)
    assert P
    for G, G0, bar, axis in ((r["Gm"], Tm, 1e-10, "iw"), (r["Gr"], Tr, 1e-8, "w")):
        scale = np.max(np.abs(G))
        for s, a, b in P:
            d = np.max(np.abs(G[s, s, a, b] - G0[s, a, b])) / scale
            dba = np.max(np.abs(G[s, s, b, a] - G0[s, b, a])) / scale
            ratio = np.max(np.abs(G[s, s, a, b])) / np.max(np.abs(G[s, s, a, a]))
            print(f"{name} G({axis}) s={s} ({a},{b}): |G_ab - truth| {d:.2e}, |G_ba - truth_ba| {dba:.2e}, "
                  f"max|G_ab|/max|G_aa| {ratio:.2f}")
            assert d < bar
            assert np.array_equal(G[s, s, b, a], G[s, s, a, b])      # the reference's plain copy
            if name != "RC":                                        # real H: the copy is the true G_ba
                assert dba < bar
            if axis == "iw":             # the off-diagonal entries are not small (every pair, G(iw))
                assert ratio > 0.1


def test_orbital_mix_off_gives_the_diagonal_alone():
    from oracle_gf import oracle_job_runner

    cfg, r = ot.truth("H3").cfg, run("H3")
    Gm, Gr = build_gf(cfg, r["sl"], gopt("H3", orbital_mix=False), runner=oracle_job_runner)
    for G, G1 in ((Gm, r["Gm"]), (Gr, r["Gr"])):
        for a in range(cfg.Norb):
            for b in range(cfg.Norb):
                if a == b:
                    assert np.any(G[:, :, a, a] != 0) and np.array_equal(G[:, :, a, a], G1[:, :, a, a])
                else:
                    assert not np.any(G[:, :, a, b])


def test_build_gf_normal_records_mixed_channels(monkeypatch):
    """build_gf_normal unpacks the channel tags of both kinds (the device path
    fills `record`; here the unpacking alone, on the tags of the job list)."""
    from edgpu import gf

    cfg, sl = ot.truth("H3").cfg, run("H3")["sl"]
    tags = {j[1] for j in _job_list(cfg, sl)[0]}
    fake = [dict(channel=t) for t in sorted(tags)]
    monkeypatch.setattr(gf, "build_gf", lambda cfg, states, gopt, device, rec: (rec.extend(fake), (None, None))[1])
    out = []
    gf.build_gf_normal(cfg, sl, None, record=out)
    assert [(r["channel"][0], r["ispin"], r["iorb"], r["jorb"]) for r in out] == \
        [(t[0], t[1], t[2], t[3] if t[0] == "orbmix" else t[2]) for t in sorted(tags)]


def _gf_worker(rank, world, port, q):
    import torch.distributed as dist
    from oracle_gf import oracle_job_runner
    from oracle_solver import solve_sector_oracle

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ot.config("H3")
    res = farm_diag(cfg, DiagOptions(lanc_method="lanczos"), solver=solve_sector_oracle)
    Gm, Gr = build_gf(cfg, res.states, gopt("H3"), owners=res.owners, runner=oracle_job_runner)
    q.put((rank, Gm, Gr))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_two_ranks_match_the_serial_build():
    """The longer job list split over 2 gloo ranks (lpt_partition, one
    all-reduce, recombination after it) equals the serial build to 1e-13."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = run("H3")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gf_worker, args=(k, 2, port, q)) for k in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, Gm, Gr in out:
        assert np.max(np.abs(Gm - r["Gm"])) / np.max(np.abs(r["Gm"])) < 1e-13
        assert np.max(np.abs(Gr - r["Gr"])) / np.max(np.abs(r["Gr"])) < 1e-13
