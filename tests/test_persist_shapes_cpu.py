"""The shape table of tests/persist_shape_cases.py against the oracle alone
(no GPU): every entry reaches the launch form it names by the host's formulas
(build_preg, pkr_geom, persist_rpt01 and persist_mode_derive's caps, restated
in geometry_from_csr / derive_mode), and the references the GPU test compares
with keep a tenth of its bars:

  * over the first m = min(24, dim // 2) steps the oracle's f64 alpha / beta,
    and those of an f64 run that sums each row last entry first, stay within
    1e-11 * max(1, max|T|) of the extended-precision recurrence (the GPU bar
    is rtol 1e-10, atol 1e-12);
  * the oracle's f64 results of the unit-vector probes stay within
    1e-13 * |H|_inf of the extended-precision ones (the GPU bar is 1e-12).

Over all min(40, dim // 2) steps of the multi-kernel comparison (bar 1e-9) the
f64 runs stay within 5e-10 of the extended-precision one.

So a change of the host formulas that moves an entry to another form, or a
sector whose recurrence loses its digits inside the window, fails here first.
"""
import numpy as np
import pytest

import persist_shape_cases as ps


@pytest.mark.parametrize("e", ps.TABLE, ids=ps.IDS)
def test_entry_reaches_its_form(e):
    csr, dim = ps.oracle_csr(e)
    assert dim == e.dim and dim >= 36
    g = ps.geometry_from_csr(csr, dim, e.hc, e.vc, e.dimup)
    assert not (g["cplx"] and not e.hc), "complex values need a complex H"
    assert g["diag_real"]
    assert ps.derive_mode(g, e) == (e.mode, e.width, e.rpt), g
    if e.mode in (1, 3, 4):
        assert g["kron"]
    if e.mode == 4:
        case = next(c for c in ps.pc.CASES if ps.pc.key(c) == e.id.split("_", 3)[3])
        assert ps.pc.geometry(case[0], *case[1]) == (g["du"], g["dd"], g["E"], g["RPT4"])
    # padding: what the form's last row slot holds
    nt = ps.nthreads(e.mode)
    assert e.rpt * nt >= dim
    if e.mode in (0, 1):
        assert (e.rpt - 1) * nt < dim or e.rpt == 8


def test_launch_entries_cover_every_case():
    got = ps.launch_entries()
    assert sorted({(e.mode, e.hc, e.vc) for e in ps.TABLE}) == [(e.mode, e.hc, e.vc) for e in got]
    for e in got:
        assert e.dim % ps.nthreads(e.mode) != 0 and e.dim > ps.nthreads(e.mode), e.id


def test_forms_are_listed_once_per_sector_kind():
    # one entry per form, plus the named second sectors of the module docstring
    forms = {}
    for e in ps.TABLE:
        forms.setdefault((ps.form(e), e.kw["stored"]), []).append(e.id)
    extra = {k: v for k, v in forms.items() if len(v) > 1}
    for ids in extra.values():
        assert len(ids) == 2 and any(("normal_jh" in i) or ("hybrid" in i) or ("nb5_3_3" in i) for i in ids), ids


@pytest.mark.parametrize("e", ps.TABLE, ids=ps.IDS)
def test_window_is_sound(e):
    r = ps.reference_run(e)
    m = r["m"]
    assert m == min(24, e.dim // 2) <= r["n"]
    ax, bx, nx = r["ext"]
    assert nx == r["n"] == r["oracle"][2] == r["rev"][2]
    scale = max(1.0, float(np.max(np.abs(ax[:m]))), float(np.max(np.abs(bx[:m]))))
    for what, (a, b, _) in (("oracle", r["oracle"]), ("reversed rows", r["rev"])):
        da = float(np.max(np.abs(np.asarray(a[:m], dtype=np.longdouble) - ax[:m])))
        db = float(np.max(np.abs(np.asarray(b[:m], dtype=np.longdouble) - bx[:m])))
        assert max(da, db) <= 1e-11 * scale, (what, da, db, scale)
    # the multi-kernel comparison runs all n = min(40, dim // 2) steps at 1e-9:
    # two f64 summation orders must not already differ by that much there (a
    # sector like nb8 (1,1), 81 rows, eight degenerate bath levels, loses
    # its digits by step 40 and is not in the table for that reason).  All
    # entries but hybrid (4,2) and replica_cplx (2,4) keep a tenth of the bar;
    # those two reach 2.2e-10 and 4.4e-10 at step 39.
    n = r["n"]
    scale = max(1.0, float(np.max(np.abs(ax[:n]))), float(np.max(np.abs(bx[:n]))))
    for what, (a, b, _) in (("oracle", r["oracle"]), ("reversed rows", r["rev"])):
        da = float(np.max(np.abs(np.asarray(a[:n], dtype=np.longdouble) - ax[:n])))
        db = float(np.max(np.abs(np.asarray(b[:n], dtype=np.longdouble) - bx[:n])))
        assert max(da, db) <= 5e-10 * scale, (what, da, db, scale)


@pytest.mark.parametrize("e", ps.TABLE, ids=ps.IDS)
def test_probes_are_sound(e):
    p = ps.reference_probes(e)
    ax, bx, nx = p["ext"]
    ao, bo, no = p["oracle"]
    assert np.array_equal(nx, no)
    tol = 1e-13 * p["hinf"]
    assert float(np.max(np.abs(ao.astype(np.longdouble) - ax))) <= tol
    assert float(np.max(np.abs(bo.astype(np.longdouble) - bx))) <= tol
    # what leg B asserts exactly: alpha[0] = H_jj, beta[1] = the column's off-diagonal norm
    assert np.array_equal(ao[:, 0], p["hjj"])
    assert float(np.max(np.abs(bx[:, 1] - p["cnorm"]))) <= 1e-17 * p["hinf"]
    cols = p["cols"]
    assert cols[0] == 0 and cols[-1] == e.dim - 1 and len(set(cols.tolist())) == len(cols)
