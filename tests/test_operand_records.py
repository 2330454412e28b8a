"""The patch-order records of elem_vertex_kernel's static per-owned-vertex operands (dot_amd/csrc/vpatches.hpp: VpOwnRec,
DOTMI_OPERAND_RECORDS) on the CPU, through the host-only entry dotmi_plan_vpatch_records: every record equals the flat arrays
gathered through the patch's vertex list -- mass, fixed, the vertex' copy count and its first four padded right-hand-side
positions (vp_ptr / vp_off) --, padding records are zero, and after a changed fixed mask the rewritten copy matches again."""
import ctypes as C

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload


def _flat_arrays(sc, ep, nparts):
    """mass, fixed and the CSR of a vertex' copies in a padded layout of the subdomains' right-hand sides: subdomain ls holds its
    vertices in ascending id, vertex i of it at ls * nmax + 3 i (nmax: the largest subdomain, padded to 64 scalars)"""
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    nV = sc.V_rest.shape[0]
    verts = [np.unique(T[ep == p]) for p in range(nparts)]
    nmax = -(-3 * max(len(v) for v in verts) // 64) * 64
    cnt = np.zeros(nV, dtype=np.int64)
    for v in verts:
        cnt[v] += 1
    vp_ptr = np.zeros(nV + 1, dtype=np.int32)
    vp_ptr[1:] = np.cumsum(cnt)
    vp_off = np.zeros(int(vp_ptr[-1]), dtype=np.int32)
    cur = vp_ptr[:-1].astype(np.int64).copy()
    for ls, v in enumerate(verts):
        vp_off[cur[v]] = ls * nmax + 3 * np.arange(len(v))
        cur[v] += 1
    mass = np.random.default_rng(3).uniform(0.5, 2.0, nV)
    fixed = np.ascontiguousarray(sc.fixed, dtype=np.uint8)
    return mass, fixed, vp_ptr, vp_off


def _records(sc, mass, fixed, vp_ptr, vp_off, fixed2=None):
    L = dl.load()
    f = L.dotmi_plan_vpatch_records
    f.argtypes = [C.c_int32, C.c_int32, dl.c_ip, dl.c_dp, C.c_int32, C.c_int32, dl.c_dp, dl.c_up, dl.c_ip, dl.c_ip, dl.c_up, dl.c_ip,
                  dl.c_ip, dl.c_ip, dl.c_dp, dl.c_ip, dl.c_ip, dl.c_ip]
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    X = np.ascontiguousarray(sc.V_rest, dtype=np.float64)
    nV, nT = X.shape[0], T.shape[0]
    hdr = np.zeros(5, dtype=np.int32)
    f2 = dl.up(fixed2) if fixed2 is not None else None
    args = (nV, nT, dl.ip(T), dl.dp(X), 512, 85, dl.dp(mass), dl.up(fixed), dl.ip(vp_ptr), dl.ip(vp_off), f2, dl.ip(hdr))
    assert f(*args, None, None, None, None, None, None) == 0
    nP, PE, PV, PO, RUN = (int(v) for v in hdr)
    assert nP > 0
    out = dict(pv_gid=np.full(nP * PV, -7, np.int32), po_cnt=np.zeros(nP, np.int32), mass=np.full(nP * PO, -1.0),
               fixed=np.full(nP * PO, -1, np.int32), cnt=np.full(nP * PO, -1, np.int32), off=np.full(4 * nP * PO, -1, np.int32))
    assert f(*args, dl.ip(out["pv_gid"]), dl.ip(out["po_cnt"]), dl.dp(out["mass"]), dl.ip(out["fixed"]), dl.ip(out["cnt"]),
             dl.ip(out["off"])) == 0
    return nP, PV, PO, out


def _check(nP, PV, PO, out, mass, fixed, vp_ptr, vp_off):
    gid = out["pv_gid"].reshape(nP, PV)
    rm, rf, rc, ro = out["mass"].reshape(nP, PO), out["fixed"].reshape(nP, PO), out["cnt"].reshape(nP, PO), out["off"].reshape(nP, PO, 4)
    owned = np.zeros(mass.size, dtype=np.int64)
    for p in range(nP):
        no = int(out["po_cnt"][p])
        assert 0 < no <= PO
        g = gid[p, :no]
        assert g.min() >= 0
        owned[g] += 1
        assert np.array_equal(rm[p, :no], mass[g])                       # bit for bit: the kernel multiplies with it
        assert np.array_equal(rf[p, :no], (fixed[g] != 0).astype(np.int32))
        assert np.array_equal(rc[p, :no], vp_ptr[g + 1] - vp_ptr[g])
        for lv, v in enumerate(g):
            k = min(4, int(rc[p, lv]))
            assert np.array_equal(ro[p, lv, :k], vp_off[vp_ptr[v]:vp_ptr[v] + k])
            assert np.all(ro[p, lv, k:] == 0)
        # behind the owned vertices: zero records (a lane there is not a vertex lane, but it loads)
        assert np.all(rm[p, no:] == 0) and np.all(rf[p, no:] == 0) and np.all(rc[p, no:] == 0) and np.all(ro[p, no:] == 0)
    assert np.all(owned == 1)                                            # every vertex has exactly one record
    return rc


@pytest.mark.parametrize("name", ["synbar:24x6x6:8", "bunny5K_LTSS"])
def test_patch_order_records_equal_the_flat_arrays_gathered_through_the_vertex_list(name):
    sc, ep, n = load_workload(name)
    assert n == 8
    mass, fixed, vp_ptr, vp_off = _flat_arrays(sc, np.asarray(ep), n)
    nP, PV, PO, out = _records(sc, mass, fixed, vp_ptr, vp_off)
    rc = _check(nP, PV, PO, out, mass, fixed, vp_ptr, vp_off)
    assert rc.max() >= 2                                                 # interface vertices: more than one copy
    if name == "bunny5K_LTSS":
        assert rc.max() > 4                                              # ... and some beyond the record's four positions
    # a changed fixed mask (dotmi_refix): the flags are rewritten, nothing else moves
    fixed2 = fixed.copy()
    fixed2[::11] ^= 1
    assert (fixed2 != fixed).any() and fixed2.any() and not fixed2.all()
    nP2, PV2, PO2, out2 = _records(sc, mass, fixed, vp_ptr, vp_off, fixed2)
    assert (nP2, PV2, PO2) == (nP, PV, PO)
    _check(nP, PV, PO, out2, mass, fixed2, vp_ptr, vp_off)
    for k in ("pv_gid", "po_cnt", "mass", "cnt", "off"):
        assert np.array_equal(out[k], out2[k]), k
    assert not np.array_equal(out["fixed"], out2["fixed"])


def test_the_records_entry_rejects_missing_arrays():
    sc, ep, n = load_workload("synbar:4x2x2:2")
    mass, fixed, vp_ptr, vp_off = _flat_arrays(sc, np.asarray(ep), n)
    L = dl.load()
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    X = np.ascontiguousarray(sc.V_rest, dtype=np.float64)
    hdr = np.zeros(5, dtype=np.int32)
    f = L.dotmi_plan_vpatch_records
    f.argtypes = [C.c_int32, C.c_int32, dl.c_ip, dl.c_dp, C.c_int32, C.c_int32, dl.c_dp, dl.c_up, dl.c_ip, dl.c_ip, dl.c_up, dl.c_ip,
                  dl.c_ip, dl.c_ip, dl.c_dp, dl.c_ip, dl.c_ip, dl.c_ip]
    assert f(X.shape[0], T.shape[0], dl.ip(T), dl.dp(X), 512, 85, None, dl.up(fixed), dl.ip(vp_ptr), dl.ip(vp_off), None, dl.ip(hdr),
             None, None, None, None, None, None) != 0
    gid = np.zeros(4096, dtype=np.int32)
    assert f(X.shape[0], T.shape[0], dl.ip(T), dl.dp(X), 512, 85, dl.dp(mass), dl.up(fixed), dl.ip(vp_ptr), dl.ip(vp_off), None,
             dl.ip(hdr), dl.ip(gid), None, None, None, None, None) != 0
