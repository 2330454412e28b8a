"""LBFGS-PD (DOTMI_FLAG_LBFGS_PD), host only: the scalar layout of the constant Laplacian L and what one application of L^-1
reads (dotmi_plan_pd), against the one-subdomain 3-dof layout LBFGS-H streams; and the 3-dof layouts left as they were."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload

ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
dpp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def _mesh(name):
    sc, ep, n = load_workload(name)
    return (np.ascontiguousarray(sc.T, dtype=np.int32), np.ascontiguousarray(sc.V_rest, dtype=np.float64),
            np.ascontiguousarray(ep, dtype=np.int32), n)


def plan_pd(T, X):
    L = dl.load()
    padded, nbytes = C.c_int32(0), C.c_int64(0)
    rc = L.dotmi_plan_pd(X.shape[0], T.shape[0], ip(T), dpp(X), C.byref(padded), C.byref(nbytes))
    assert rc == 0
    return padded.value, nbytes.value


def one_subdomain_bytes(T, X):
    L = dl.load()
    ep = np.zeros(T.shape[0], dtype=np.int32)
    f, b = C.c_int32(-1), C.c_int64(0)
    L.dotmi_plan_backsolve_form.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                            C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    rc = L.dotmi_plan_backsolve_form(X.shape[0], T.shape[0], ip(T), dpp(X), ip(ep), 1, C.byref(f), C.byref(b))
    assert rc == 0
    return b.value


@pytest.mark.parametrize("name", ["bunny5K_LTSS", "bar17K_twist", "monkey18K_TSS_1K"])
def test_scalar_factor_streams_at_most_a_sixth_of_the_block_factor(name):
    """The Kronecker structure L (x) I_3 alone costs 9x the bytes of the scalar factor; the bar leaves room for the padding of
    the scalar layout and for the blocks whose rows the apply kernel reads twice."""
    T, X, _, _ = _mesh(name)
    padded, pd_bytes = plan_pd(T, X)
    assert padded % 64 == 0 and padded >= X.shape[0]
    block = one_subdomain_bytes(T, X)
    assert 0 < pd_bytes <= block / 6, (pd_bytes, block)


def test_plan_pd_rejects_bad_meshes():
    L = dl.load()
    T = np.array([[0, 1, 2, 7]], dtype=np.int32)
    X = np.zeros((4, 3))
    padded, nbytes = C.c_int32(0), C.c_int64(0)
    assert L.dotmi_plan_pd(4, 1, ip(T), dpp(X), C.byref(padded), C.byref(nbytes)) < 0   # vertex 7 of 4
    assert L.dotmi_plan_pd(0, 1, ip(T), dpp(X), C.byref(padded), C.byref(nbytes)) < 0


# dotmi_plan_layout of the BASELINE workloads (nodes, padded size, positions), recorded on the tree before LBFGS-PD gave the
# dissection its unknowns-per-vertex parameter
LAYOUT_DIGESTS = {"bunny5K_LTSS": "0237dd1e9a0e59b3", "bar17K_twist": "0f7c1039eb0c96f4", "horse7K_stretch": "b25e5540eb879c17",
                  "monkey18K_stiff": "b5e2e1037c75e186", "kingkong18K_SS_1K": "0bc891e3abb34fe9"}


@pytest.mark.parametrize("name", ["bunny5K_LTSS", "bar17K_twist", "horse7K_stretch", "monkey18K_stiff", "kingkong18K_SS_1K"])
def test_block_layouts_are_unchanged(name):
    from dot_amd.sharding import plan_layout
    old = os.environ.pop("DOTMI_TWO_LEVEL", None)
    try:
        T, X, ep, n = _mesh(name)
        nodes, nmax, pos, _ = plan_layout(X, T, ep, n)
    finally:
        if old is not None:
            os.environ["DOTMI_TWO_LEVEL"] = old
    h = hashlib.sha256(nodes.tobytes() + np.int64(nmax).tobytes() + b"".join(p.tobytes() for p in pos)).hexdigest()[:16]
    assert h == LAYOUT_DIGESTS[name], h


def test_runner_writes_no_partition_files_for_lbfgs_pd(tmp_path):
    """dot_hip on a `timeStepper LBFGS` script (host only, --dump-scene): the whole mesh, no partition, and none of the partition
    files a DOT script gets (label.obj / wire.poly: the ADMMDD constructor's)"""
    import subprocess
    from tests.test_host_logic import _write_msh
    from dot_amd import scene
    from dot_amd.workloads import MESH_DIR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "dot_amd", "host")])
    V, T = scene.load_mesh_npz(os.path.join(MESH_DIR, "bunny5K.npz"))
    _write_msh(tmp_path / "bunny5K.msh", V, T)
    body = "energy FCR\nsize 1\ntime 5 0.025\ndensity 1000\nstiffness 100000 0.4\nscript twistnsns\nshape input bunny5K.msh\n"
    for stepper, parts in (("DOT 8", True), ("LBFGS", False)):
        (tmp_path / "s.txt").write_text(f"timeStepper {stepper}\n" + body)
        o = tmp_path / stepper.split()[0]
        subprocess.check_call([exe, "100", str(tmp_path / "s.txt"), "--mesh-root", str(tmp_path), "--dump-scene", "1", "--out", str(o)],
                              stdout=subprocess.DEVNULL, timeout=600)
        assert (o / "label.obj").exists() == parts and (o / "wire.poly").exists() == parts, stepper
