"""Sectors and runs shared by tests/test_gpu_persist_mode4.py and the script
that records its fixture (tests/golden/make_persist_mode4_parent.py).

Norb=1 normal-mode sectors, the smallest that reach each code shape of the
persistent Kronecker-register Lanczos kernel (MODE 4, real vectors): hop-list
width E and rows per thread RPT as pkr_geom (csrc/ed_lanczos.hip) derives them
from DimUp x DimDw and the hop degrees.
"""
from math import comb

import numpy as np

NT = 512          # kPRegBlock: threads of the MODE 4 workgroup
NSTEP = 60        # recorded Lanczos steps (fewer in sectors smaller than that)
NBATCH = 3        # start vectors of the batched leg
# lanc_eigh runs the persistent kernel in launches of 64 steps and tests
# convergence on the host between them: no Ritz test before step 70 and a zero
# tolerance, so the run takes at least the second launch (the continuation
# path: first = 0, R and P reloaded from memory)
EIGH_KW = dict(nitermax=80, threshold=0.0, ncheck=70)

# (Nbath, (nup, ndw), (DimUp, DimDw), E, RPT, software-pipelined loop)
CASES = [
    (3, (2, 2), (6, 6), 4, 2, True),      # idle lanes and padding slots
    (5, (3, 3), (20, 20), 4, 2, True),
    (6, (3, 3), (35, 35), 4, 4, True),
    (7, (2, 2), (28, 28), 8, 2, True),
    (7, (3, 2), (56, 28), 8, 4, True),
    (7, (4, 4), (70, 70), 4, 10, True),   # configs[1]: the benchmark's sector
    (8, (3, 2), (84, 36), 8, 6, False),   # RPT * E > 40: the plain row loop
]
IDS = ["nb%d_%d_%d" % (c[0], c[1][0], c[1][1]) for c in CASES]
# legs beyond the plain run: continuation launches, batch, kept Krylov basis
LEG_CASES = [c for c in CASES if c[:2] in ((5, (3, 3)), (7, (4, 4)))]
LEG_IDS = ["nb%d_%d_%d" % (c[0], c[1][0], c[1][1]) for c in LEG_CASES]


def key(case):
    return "nb%d_%d_%d" % (case[0], case[1][0], case[1][1])


def geometry(nbath, nup, ndw):
    """(DimUp, DimDw, E, RPT) by pkr_geom's formulas.  Star geometry: a spin
    configuration with q electrons on Ns = Nbath + 1 levels has q hops when
    the impurity is empty and Nbath - (q - 1) when it is occupied."""
    ns = nbath + 1
    du, dd = comb(ns, nup), comb(ns, ndw)

    def deg(q):
        return max(q if q <= nbath else 0, nbath - (q - 1) if q >= 1 else 0)

    d = max(deg(nup), deg(ndw))
    e = 4 if d <= 4 else 8
    g = NT // du
    rpt = (dd + g - 1) // g
    rpt = next(r for r in (2, 4, 6, 8, 10) if rpt <= r)
    return du, dd, e, rpt


def start(dim, k=1):
    return np.sin(k * np.arange(1, dim + 1, dtype=np.float64))


def nsteps(dim):
    return min(NSTEP, dim)


def open_sector(case, options=()):
    from edgpu.hamiltonian import Sector
    from edgpu.params import make_config

    cfg = make_config(Norb=1, Nbath=case[0])
    return Sector(cfg, case[1][0], case[1][1], stored=True, real=True, options=options)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
