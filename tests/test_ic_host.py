"""LBFGS-HI (DOTMI_FLAG_LBFGS_HI), host only: the multicolour plan of the block incomplete Cholesky (dotmi_plan_ic) and its numpy
restatement (tests/ic_reference.py) -- the defining property of IC(0), the shift policy with its 40-attempt cap, and the vectorised
restatement against the same arithmetic one vertex at a time, both driving the oracle."""
import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload
from tests import ic_reference as R

MESHES = ["synbar:16x5x5:1", "bunny5K_LTSS"]
_plans = {}


def plan_of(name):
    if name not in _plans:
        sc, _, _ = load_workload(name)
        _plans[name] = (sc, R.plan_ic(sc.T, sc.V_rest.shape[0]))
    return _plans[name]


@pytest.mark.parametrize("name,colours", [("synbar:16x5x5:1", 8), ("bunny5K_LTSS", 12)])
def test_colouring_is_proper_greedy_and_ordered(name, colours):
    sc, P = plan_of(name)
    nV = P["nV"]
    ptr, idx = R.adjacency(sc.T, nV)
    col, pos = P["colour"], P["pos"]
    assert P["nColours"] == colours == col.max() + 1 and col.min() == 0
    rows = np.repeat(np.arange(nV), np.diff(ptr))
    off = rows != idx
    assert (col[rows[off]] != col[idx[off]]).all()          # no edge inside a colour
    # greedy in ascending vertex id: every smaller colour is held by an earlier neighbour
    for v in range(nV):
        nb = idx[ptr[v]:ptr[v + 1]]
        assert set(range(col[v])) <= set(col[nb[nb < v]]), v
    # order by (colour, vertex id)
    assert sorted(pos) == list(range(nV))
    order = np.argsort(pos)
    key = col[order].astype(np.int64) * nV + order
    assert (np.diff(key) > 0).all()


@pytest.mark.parametrize("name", MESHES)
def test_every_lower_block_appears_exactly_once(name):
    sc, P = plan_of(name)
    nV, nL = P["nV"], P["nL"]
    ptr, idx = R.adjacency(sc.T, nV)
    pos, lptr, lidx, lsrc, dsrc = P["pos"], P["lptr"], P["lidx"], P["lsrc"], P["dsrc"]
    vert = np.argsort(pos)
    rows = np.repeat(np.arange(nV), np.diff(ptr))
    lower = pos[idx] < pos[rows]                             # the entries of H's pattern below the diagonal of the new order
    assert nL == lower.sum() == (len(idx) - nV) // 2
    rowp = np.repeat(np.arange(nV), np.diff(lptr))
    assert (lidx < rowp).all()
    for p in range(nV):
        assert (np.diff(lidx[lptr[p]:lptr[p + 1]]) > 0).all(), p   # ascending, so no block twice
    # a lower block's source is the CSR entry (its row's vertex, its column's vertex); the diagonal's likewise
    assert (rows[lsrc] == vert[rowp]).all() and (idx[lsrc] == vert[lidx]).all()
    assert len(set(lsrc.tolist())) == nL and set(lsrc.tolist()) == set(np.nonzero(lower)[0].tolist())
    assert (rows[dsrc] == vert).all() and (idx[dsrc] == vert).all()


@pytest.mark.parametrize("name", MESHES)
def test_product_lists_name_existing_blocks_in_ascending_order(name):
    sc, P = plan_of(name)
    nV, nL = P["nV"], P["nL"]
    lptr, lidx, pptr, pa, pb = P["lptr"], P["lidx"], P["pptr"], P["pa"], P["pb"]
    assert pptr[0] == 0 and pptr[-1] == P["nP"] == len(pa) == len(pb) and (np.diff(pptr) >= 0).all()
    rowp = np.repeat(np.arange(nV), np.diff(lptr))
    blk = np.repeat(np.arange(nL), np.diff(pptr))            # the block every product belongs to
    i, j = rowp[blk], lidx[blk]
    # pa: a block of row i in front of (i, j); pb: a block of row j; both on the same column k
    assert (pa >= lptr[i]).all() and (pa < blk).all()
    assert (pb >= lptr[j]).all() and (pb < lptr[j + 1]).all()
    assert (lidx[pa] == lidx[pb]).all()
    same = blk[1:] == blk[:-1]
    assert (np.diff(lidx[pa])[same] > 0).all()
    # and complete: exactly the common lower neighbours
    lowers = [set(lidx[lptr[p]:lptr[p + 1]].tolist()) for p in range(nV)]
    cnt = np.diff(pptr)
    for s in range(nL):
        assert cnt[s] == len(lowers[rowp[s]] & lowers[lidx[s]]), s


def random_spd_blocks(sc, seed=0):
    """a symmetric block matrix on the mesh's pattern, strictly block-diagonally dominant: (nnzb, 3, 3) in CSR order + dense"""
    nV = sc.V_rest.shape[0]
    ptr, idx = R.adjacency(sc.T, nV)
    rows = np.repeat(np.arange(nV), np.diff(ptr))
    rng = np.random.default_rng(seed)
    A = np.zeros((3 * nV, 3 * nV))
    for r, c in zip(rows, idx):
        if c < r:
            B = rng.standard_normal((3, 3))
            A[3 * r:3 * r + 3, 3 * c:3 * c + 3] = B
            A[3 * c:3 * c + 3, 3 * r:3 * r + 3] = B.T
    A += np.diag(np.abs(A).sum(axis=1) + rng.uniform(0.5, 1.5, 3 * nV))
    blocks = np.stack([A[3 * r:3 * r + 3, 3 * c:3 * c + 3] for r, c in zip(rows, idx)])
    return blocks, A, rows, idx


def test_factor_reproduces_the_matrix_on_its_pattern():
    """the defining property of IC(0): (L L^T)_ij = A_ij on every position of the pattern, to 1e-12 relative"""
    sc, P = plan_of("synbar:16x5x5:1")
    blocks, A, rows, idx = random_spd_blocks(sc)
    ref = R.ICReference(P)
    assert ref.factor(blocks) and ref.shift == 0.0 and ref.attempts == 1
    LLt = ref.dense_product()
    got = np.stack([LLt[3 * r:3 * r + 3, 3 * c:3 * c + 3] for r, c in zip(rows, idx)])
    err = np.abs(got - blocks).reshape(len(idx), -1).max(axis=1)
    assert (err <= 1e-12 * np.abs(blocks).reshape(len(idx), -1).max(axis=1)).all(), err.max()
    # (incomplete: off the pattern L L^T has fill that A does not)
    mask = np.ones_like(A, dtype=bool)
    for r, c in zip(rows, idx):
        mask[3 * r:3 * r + 3, 3 * c:3 * c + 3] = False
    assert np.abs(LLt[mask]).max() > 1e-3
    # the solve is the inverse of that product
    b = np.random.default_rng(1).standard_normal((P["nV"], 3))
    x = ref.solve(b)
    assert np.abs(LLt @ x.ravel() - b.ravel()).max() <= 1e-10 * np.abs(b).max()


class ThresholdReference(R.ICReference):
    """the shift policy alone: an attempt succeeds from a given shift on"""

    def __init__(self, thr):
        self.shift, self.attempts, self.F, self.thr, self.tried = 0.0, 0, None, thr, []

    def factor_attempt(self, blocks, sigma):
        self.tried.append(sigma)
        return None, sigma >= self.thr


def test_shift_policy_halves_then_doubles_and_stops_at_forty_attempts():
    ref = ThresholdReference(0.1)
    assert ref.factor(None)
    assert ref.tried == [0.0] + [1e-3 * 2 ** k for k in range(8)] and ref.shift == 0.128 and ref.attempts == 9
    ref.tried = []
    assert ref.factor(None)                      # half the last shift fails, the doubled one is the last shift again
    assert ref.tried == [0.064, 0.128] and ref.attempts == 2
    ref.thr, ref.tried = 0.01, []
    assert ref.factor(None) and ref.tried == [0.064] and ref.shift == 0.064 and ref.attempts == 1
    ref.thr, ref.tried = 0.0, []
    for _ in range(3):
        assert ref.factor(None)
    assert ref.tried == [0.032, 0.016, 0.008]    # (never back to exactly 0 once a shift was needed)
    never = ThresholdReference(np.inf)
    assert not never.factor(None) and len(never.tried) == 40 == never.attempts and never.shift == 0.0
    assert never.tried[1] == 1e-3 and never.tried[-1] == 1e-3 * 2 ** 38


def test_indefinite_matrix_exhausts_the_attempts():
    sc, P = plan_of("synbar:16x5x5:1")
    blocks, _, rows, idx = random_spd_blocks(sc)
    ref = R.ICReference(P)
    assert not ref.factor(-blocks) and ref.attempts == 40 and ref.F is None


def run_oracle(energy, loop, nsteps):
    sc, _, _ = load_workload("synbar:16x5x5:1")
    ref = R.ICReference(plan_of("synbar:16x5x5:1")[1], loop=loop)
    sol = R.ICSolver(ref)
    orc = R.oracle_whole_mesh(sc, energy)
    sol.bind(orc)
    its = []
    for k in range(nsteps):
        idx, pos = sc.scripter.step(orc.state()[0], sc.cfg.dt)
        orc.move(idx, pos)
        so = orc.step()
        assert so.status == 0
        its.append((so.iters, so.ls_halvings))
    out = its, ref.F.copy(), orc.state()[0].copy(), list(sol.log)
    orc.close()
    return out


@pytest.mark.parametrize("energy", [dl.ENERGY_FCR, dl.ENERGY_SNH])
def test_oracle_iterations_on_the_small_bar(energy):
    """four scripted steps of the small bar with the restatement as the oracle's solver: 9, 12, 14, 14 iterations for both
    materials, the factorisation at the binding and one per step, none of them shifted"""
    its, _, _, log = run_oracle(energy, False, 4)
    assert [i for i, _ in its] == [9, 12, 14, 14]
    assert log == [(0.0, 1)] * 5


def test_oracle_takes_the_same_iterations_with_the_per_vertex_loop():
    """the vectorised restatement against the same arithmetic one vertex at a time, each driving the oracle through two scripted
    steps (the loop takes ~3 s per step): the same iterations -- and, the operations being the same, bit-identical factors and
    positions"""
    a, b = run_oracle(dl.ENERGY_FCR, False, 2), run_oracle(dl.ENERGY_FCR, True, 2)
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_runner_takes_lbfgs_hi_as_the_whole_mesh(tmp_path):
    """dot_hip on a `timeStepper LBFGSHI` script (host only, --dump-scene): the whole mesh, no partition, none of the partition
    files a DOT script gets"""
    import os
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
    (tmp_path / "s.txt").write_text("timeStepper LBFGSHI\n" + body)
    o = tmp_path / "hi"
    subprocess.check_call([exe, "100", str(tmp_path / "s.txt"), "--mesh-root", str(tmp_path), "--dump-scene", "1", "--out", str(o)],
                          stdout=subprocess.DEVNULL, timeout=600)
    assert o.exists() and not (o / "label.obj").exists() and not (o / "wire.poly").exists()
