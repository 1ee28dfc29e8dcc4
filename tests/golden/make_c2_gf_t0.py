"""Record tests/golden/c2_gf_t0.npz: the T=0 Green's function of configs[1]
(Norb=1, Nbath=7, random bath of seed 20251015) from its ground-state sector
(4,4) alone, DiagOptions() and GFOptions(Lmats=16, Lreal=16) otherwise at
their defaults: E0, Gm and Gr (1, 1, 1, 1, 16) complex.

The committed file was recorded with the Python package of the commit BEFORE
the finite-temperature state list (lanc_nstates_total, ed_twin) was added, on
the library of the commit that added it (whose Green's-function kernels are
the same); tests/test_gpu_finite_t.py compares later builds with it bit for
bit: the default options must keep computing exactly the T=0 numbers,
weights norm2 / len(states) included.  Two runs in one process gave the same
bits.  Re-record only when a change of the T=0 arithmetic is intended.

Needs the MI355X:  python tests/golden/make_c2_gf_t0.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "dmft-ed_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    from edgpu.diag import DiagOptions, ed_diag
    from edgpu.gf import GFOptions, build_gf
    from edgpu.params import make_config
    from edgpu.sectors import get_sector

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "c2_gf_t0.npz")
    cfg = make_config(Norb=1, Nbath=7, bath="random", seed=20251015)
    runs = []
    for _ in range(2):
        _, sl = ed_diag(cfg, DiagOptions(), sectors=[get_sector(cfg)[(4, 4)].isector])
        Gm, Gr = build_gf(cfg, sl, GFOptions(Lmats=16, Lreal=16))
        runs.append((sl.energies[0], Gm, Gr))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    np.savez(out, E0=np.float64(runs[0][0]), Gm=runs[0][1], Gr=runs[0][2])
    print("wrote", out, "E0 =", repr(runs[0][0]))


if __name__ == "__main__":
    main()
