"""Record tests/golden/persist_mode4_parent.npz: alpha and beta of the
persistent MODE 4 Lanczos kernel (real vectors) for the sectors of
tests/persist_mode4_cases.py, as the library built from the commit BEFORE a
change to that kernel computes them.  tests/test_gpu_persist_mode4.py compares
later builds with these bit for bit: a change of the kernel's instruction
stream or schedule must not change or move a floating-point operation.

Needs the MI355X (it runs the kernel):
    python tests/golden/make_persist_mode4_parent.py [out.npz]

Per sector: a_<key>, b_<key> (lanc_tridiag, min(60, dim) steps, v0 = sin(1..dim))
and, for the two sectors with further legs, e0_<key>, ne_<key>: the energy and
step count of lanc_eigh (persist_mode4_cases.EIGH_KW), whose 64-step launches
take the continuation path.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "dmft-ed_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import persist_mode4_cases as pc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "persist_mode4_parent.npz")
    rec = {}
    for case in pc.CASES:
        k = pc.key(case)
        with pc.open_sector(case) as S:
            mode = S.lanc_mode(real=True)
            geo = pc.geometry(case[0], *case[1])
            assert (int(S.info.dimup), int(S.info.dimdw)) == geo[:2] == case[2], (k, geo)
            assert geo[2:] == case[3:5], (k, geo)
            assert mode == 4, (k, mode)
            n = pc.nsteps(S.dim)
            v0 = pc.start(S.dim)
            a, b, ng = S.lanc_tridiag(v0, n)
            rec["a_" + k], rec["b_" + k], rec["n_" + k] = a, b, np.int64(ng)
            # how far the multi-kernel recurrence follows (printed, not stored)
            S.set_options("no_persist")
            a2, b2, n2 = S.lanc_tridiag(v0, n)
            S.set_options()
            m = min(ng, n2)
            da = np.abs(a[:m] - a2[:m]) / (1e-11 / 1e-9 + np.abs(a2[:m]))
            db = np.abs(b[:m] - b2[:m]) / (1e-11 / 1e-9 + np.abs(b2[:m]))
            bad = np.nonzero(np.maximum(da, db) > 1e-9)[0]
            print(f"{k}: dim={S.dim} mode={mode} geo={geo} steps={ng}/{n2} "
                  f"first step off the multi-kernel run by > 1e-9: {bad[0] if len(bad) else None} "
                  f"min beta[1:]={b[1:ng].min() if ng > 1 else None:.3e} at {1 + int(np.argmin(b[1:ng])) if ng > 1 else None}",
                  flush=True)
            if case in pc.LEG_CASES:
                e0, vec, ne = S.lanc_eigh(v0=v0, **pc.EIGH_KW)
                rec["e0_" + k], rec["ne_" + k] = np.float64(e0), np.int64(ne)
                res = np.linalg.norm(S.hxv(vec.astype(np.complex128)) - e0 * vec)
                print(f"{k}: lanc_eigh e0={e0!r} steps={ne} residual={res:.3e} "
                      f"|vec|-1={np.linalg.norm(vec) - 1.0:.2e}", flush=True)
    np.savez(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
