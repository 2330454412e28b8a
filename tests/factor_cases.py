"""The cases of tests/test_gpu_factor_accuracy.py and what the host side says about them (no GPU; checked by
tests/test_factor_reference.py): small meshes, designed matrices, the arithmetically distinct forms of the tile factorisation.

MESHES.  Synthetic bars in the workload syntax (synbar:AxBxC:parts):
  2x1x1          one tile, mostly padding (36 live rows of 64)
  8x3x3          several tile columns per part, one dissection split
  16x5x5         a deeper dissection (a case of tests/backsolve_cases.py as well)
  8x3x3-unequal  a hand-made epart of three very unequal parts, one of them a single tet: a shared padded layout, padding-only tiles
  8x3x3-free     no fixed vertex: every subdomain floats, its rigid modes are held by the mass term alone
MATRICES, all through the existing ABI on the one handle of a (mesh, switch set), in this order:
  rest           as created
  twist          updatePrecondMtrAndFactorize at an analytic twist (0.8 rad over the length) and stretch (1.3) of the rest positions
  line           ... at the "line" crush of tests/test_gpu_designed_states.py: the projection is active in every tet
  lame1e4        setLame: mu and lambda of every other element times 1e4, at rest
  pr049          setLame: PR = 0.49, at rest
  dt1e-4, dt1    setLame back to the scene's, then setTime(dt): the factors built with the old dt are stale and must be rebuilt
KAPPA lists, per mesh and matrix, the largest 2-norm condition number among its H_s (numpy, from the oracle's doubles); all stay far
below 1e10, so that max B <= 1e-7 can hold (tests/factor_reference.py).
SWITCHES.  Levels, dataflow and split levels, each with both diagonal forms; on the levels form also the eager groupings and the
cleared-and-filled H tiles.  All with DOTMI_TWO_LEVEL=0: the two-level form has no explicit X_s (out of scope)."""
import numpy as np

from tests import factor_reference as FR

MESHES = {
    "2x1x1": ("synbar:2x1x1:1", "rcb", True),
    "8x3x3": ("synbar:8x3x3:4", "rcb", True),
    "16x5x5": ("synbar:16x5x5:4", "rcb", True),
    "8x3x3-unequal": ("synbar:8x3x3:3", "unequal", True),
    "8x3x3-free": ("synbar:8x3x3:4", "rcb", False),
}
ALL_MATRICES = ("rest", "twist", "line", "lame1e4", "pr049", "dt1e-4", "dt1")
MATRICES = {m: ALL_MATRICES for m in MESHES}

_LEVELS = {"DOTMI_TILE_FLOW": "0", "DOTMI_TILE_SPLIT": "0"}
_SPLIT = {"DOTMI_TILE_FLOW": "0", "DOTMI_TILE_SPLIT": "1"}
# name -> (environment, factor kind of dotmi_factor_kind: 1 levels, 2 dataflow, 3 split levels)
SWITCHES = {
    "levels": (dict(_LEVELS), 1),
    "levels-slowdiag": (dict(_LEVELS, DOTMI_FAST_DIAG="0"), 1),
    "flow": ({"DOTMI_TILE_FLOW": "1"}, 2),
    "flow-slowdiag": ({"DOTMI_TILE_FLOW": "1", "DOTMI_FAST_DIAG": "0"}, 2),
    "split": (dict(_SPLIT), 3),
    "split-slowdiag": (dict(_SPLIT, DOTMI_FAST_DIAG="0"), 3),
    "levels-eager1": (dict(_LEVELS, DOTMI_TILE_EAGER_MIN="1"), 1),
    "levels-eager1000": (dict(_LEVELS, DOTMI_TILE_EAGER_MIN="1000"), 1),
    "levels-rmul0": (dict(_LEVELS, DOTMI_TILE_EAGER_MIN_RMUL="0"), 1),
    "levels-nohfill": (dict(_LEVELS, DOTMI_TILE_HFILL="0"), 1),
}
# (eager_min, eager_chunk) the host-only entry dotmi_plan_tile_schedule is asked for: the product's rule for few tile columns
# (plan_factor_schedule: 2 / 2) and the two settings of the switch sets.  The entry keeps as many early products in a TP_RMUL task as
# in any other (the product keeps one, or none with DOTMI_TILE_EAGER_MIN_RMUL=0): a grouping of the same sums, which the bound
# does not depend on.
EAGER = {"default": (2, 2), "eager1": (1, 2), "eager1000": (1000, 2)}

# kappa_2(H_s), the largest over the subdomains, per mesh and matrix (computed by kappa() below; test_factor_reference.py re-computes
# and compares to 10 %)
KAPPA = {
    "2x1x1": {"rest": 106.0, "twist": 163.0, "line": 118.0, "lame1e4": 5.19e5, "pr049": 905.0, "dt1e-4": 10.4, "dt1": 1.57e5},
    "8x3x3": {"rest": 113.0, "twist": 153.0, "line": 88.3, "lame1e4": 4.22e5, "pr049": 1060.0, "dt1e-4": 6.91, "dt1": 1.33e5},
    "16x5x5": {"rest": 238.0, "twist": 289.0, "line": 171.0, "lame1e4": 2.44e5, "pr049": 2270.0, "dt1e-4": 38.4, "dt1": 7.76e4},
    "8x3x3-unequal": {"rest": 191.0, "twist": 234.0, "line": 149.0, "lame1e4": 4.39e5, "pr049": 1780.0, "dt1e-4": 6.91, "dt1": 1.38e5},
    "8x3x3-free": {"rest": 263.0, "twist": 280.0, "line": 172.0, "lame1e4": 2.99e5, "pr049": 2180.0, "dt1e-4": 12.0, "dt1": 1560.0},
}


def unequal_epart(sc):
    """three parts of an 8x3x3 bar: part 0 a single tet (the one nearest the bar's far corner); part 1 the tets whose centroid lies
    in the first eighth of the length and the seven next ones along the bar (36 vertices: 30, 51 and 27 live rows in its three live
    tiles, so identity padding starts inside a 4 x 4 block in each); part 2 all the rest"""
    V, T = np.asarray(sc.V_rest), np.asarray(sc.T)
    cen = V[T].mean(axis=1)
    x0, x1 = V[:, 0].min(), V[:, 0].max()
    along = np.argsort(cen[:, 0] + 1e-3 * cen[:, 1] + 1e-6 * cen[:, 2], kind="stable")
    ep = np.full(T.shape[0], 2, dtype=np.int32)
    ep[along[:int((cen[:, 0] < x0 + (x1 - x0) / 8).sum()) + 7]] = 1
    ep[int(np.argmax(cen.sum(axis=1)))] = 0
    return ep


def twist_and_stretch(V):
    V = np.asarray(V, dtype=np.float64)
    c = (V.min(axis=0) + V.max(axis=0)) / 2
    s = (V[:, 0] - V[:, 0].min()) / (V[:, 0].max() - V[:, 0].min())
    th = 0.8 * s
    y, z = V[:, 1] - c[1], V[:, 2] - c[2]
    x = np.empty_like(V)
    x[:, 0] = V[:, 0].min() + 1.3 * (V[:, 0] - V[:, 0].min())
    x[:, 1] = c[1] + np.cos(th) * y - np.sin(th) * z
    x[:, 2] = c[2] + np.sin(th) * y + np.cos(th) * z
    return x


def line_crush(sc):
    from tests.test_gpu_designed_states import crushed_start
    return np.array(crushed_start(sc, "line"), dtype=np.float64)


class Mesh:
    """a mesh of MESHES: scene, partition, layouts, and per matrix (positions, mu, lambda, dt)"""

    def __init__(self, name):
        from dot_amd.scene import lame
        from dot_amd.sharding import plan_layout
        from dot_amd.workloads import load_workload
        workload, part, fixed = MESHES[name]
        self.name = name
        self.sc, ep, self.nparts = load_workload(workload)
        if not fixed:
            self.sc.scripter.fixed[:] = 0
        self.ep = unequal_epart(self.sc) if part == "unequal" else ep
        sc = self.sc
        self.nodes, self.nmax, self.pos, self.verts = plan_layout(sc.V_rest, sc.T, self.ep, self.nparts)
        self.layouts = [FR.Layout(sc.T, self.verts[p], self.pos[p], self.nmax) for p in range(self.nparts)]
        nT = sc.T.shape[0]
        mu0, lam0 = lame(sc.cfg.YM, sc.cfg.PR)
        mu49, lam49 = lame(sc.cfg.YM, 0.49)
        self.base = (np.full(nT, mu0), np.full(nT, lam0))
        alt = np.where(np.arange(nT) % 2 == 1, 1e4, 1.0)
        x0 = np.array(sc.x0, dtype=np.float64)
        dt = sc.cfg.dt
        self.config = {
            "rest": (x0, *self.base, dt),
            "twist": (twist_and_stretch(sc.V_rest), *self.base, dt),
            "line": (line_crush(sc), *self.base, dt),
            "lame1e4": (x0, mu0 * alt, lam0 * alt, dt),
            "pr049": (x0, np.full(nT, mu49), np.full(nT, lam49), dt),
            "dt1e-4": (x0, *self.base, 1e-4),
            "dt1": (x0, *self.base, 1.0),
        }
        self.matrices = MATRICES[name]
        self._oracle = {}
        self._plans = {}
        self._kinds = {}

    def oracle_H(self, matrix):
        """[H_s per part] from the CPU oracle (tests/oracle_py.OracleSim.part_dense), ascending vertex order"""
        if matrix not in self._oracle:
            from tests import oracle_py as O
            sc, cfg = self.sc, self.sc.cfg
            x, mu, lam, dt = self.config[matrix]
            orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, dt, sc.fixed, sc.x0, self.ep, self.nparts,
                              cfg.with_gravity, mu=mu, lam=lam)
            try:
                orc.refactor(x)
                for p in range(self.nparts):
                    assert np.array_equal(orc.part_verts(p), self.verts[p])
                self._oracle[matrix] = [orc.part_dense(p) for p in range(self.nparts)]
            finally:
                orc.close()
        return self._oracle[matrix]

    def plan(self, part, eager="default"):
        """the task list of the part's tile pattern from the host-only planner (tests/test_tile_schedule.plan, every row block stored
        from tile column 0)"""
        if (part, eager) not in self._plans:
            from tests.test_tile_schedule import plan
            lay = self.layouts[part]
            self._plans[part, eager] = plan(lay.nt, lay.live, lay.hpat, np.zeros(lay.nt, dtype=np.int32), *EAGER[eager])
        return self._plans[part, eager]

    def device_task_kinds(self, switches):
        """{(form, post): tasks} per part of the task list dotmi_create plans for this mesh under a switch set's environment: the host-only
        entry dotmi_plan_tile_fill_mesh, which runs the product's own stages (layout, rows, storage, fill lists,
        plan_factor_schedule with its eager rules) -- the list the handle of the GPU test executes, whatever kernel form runs it"""
        import ctypes as C
        import os

        from dot_amd import lib as dl
        if switches not in self._kinds:
            env = SWITCHES[switches][0]
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                sc = self.sc
                f = C.CDLL(dl.LIB_PATH).dotmi_plan_tile_fill_mesh
                i32, i64, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
                f.argtypes = [C.c_int32, C.c_int32, i32, f64, i32, C.c_int32, C.c_int32, C.c_int32, i64, i64, i64, i32, i32, i64, i32, i64]
                T = np.ascontiguousarray(sc.T, dtype=np.int32)
                X = np.ascontiguousarray(sc.V_rest, dtype=np.float64)
                ep = np.ascontiguousarray(self.ep, dtype=np.int32)
                counts = np.zeros(8, dtype=np.int64)
                head = (X.shape[0], T.shape[0], T.ctypes.data_as(i32), X.ctypes.data_as(f64), ep.ctypes.data_as(i32), self.nparts, 1, 0,
                        counts.ctypes.data_as(i64))
                assert f(*head, None, None, None, None, None, None, None) == 1
                tasks = np.zeros((counts[0], 10), dtype=np.int64)
                clear = np.zeros((counts[1], 5), dtype=np.int64)
                pos, src = np.zeros(counts[2], dtype=np.int32), np.zeros(counts[2], dtype=np.int32)
                dst, srcs = np.zeros(9 * counts[3], dtype=np.int64), np.zeros(counts[3], dtype=np.int32)
                pad = np.zeros(counts[4], dtype=np.int64)
                assert f(*head, tasks.ctypes.data_as(i64), clear.ctypes.data_as(i64), pos.ctypes.data_as(i32), src.ctypes.data_as(i32),
                         dst.ctypes.data_as(i64), srcs.ctypes.data_as(i32), pad.ctypes.data_as(i64)) == 1
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            from collections import Counter
            kinds = [Counter() for _ in range(self.nparts)]
            for _, _, block, _, _, _, post, _, _, form in tasks.tolist():
                kinds[block][("FACT" if form == FR.TF_FACT else "INV", FR.POST_NAME[post])] += 1
            self._kinds[switches] = kinds
        return self._kinds[switches]

    def lmax(self):
        """the most products one tile receives, over the parts (the same for every eager setting: the grouping moves, the sum stays)"""
        return max(FR.most_products(self.plan(p)) for p in range(self.nparts))


_meshes = {}


def mesh(name):
    if name not in _meshes:
        _meshes[name] = Mesh(name)
    return _meshes[name]


_refs = {}


def references(mesh_name, matrices, H_by_matrix=None):
    """{matrix: [Reference per part]}; H_by_matrix[matrix] = the doubles per part to build them from (dissection order is applied
    here), default the oracle's.  Cached per (mesh, matrix) as long as the doubles are the same bit for bit; what is missing is
    computed on up to eight threads (the longdouble products release the interpreter)."""
    from concurrent.futures import ThreadPoolExecutor
    m = mesh(mesh_name)
    Hs = {k: (m.oracle_H(k) if H_by_matrix is None else H_by_matrix[k]) for k in matrices}
    todo = []
    for k in matrices:
        hit = _refs.get((mesh_name, k))
        if hit is None or not all(np.array_equal(a, b) for a, b in zip(hit[0], Hs[k])):
            _refs[mesh_name, k] = ([np.array(h) for h in Hs[k]], [None] * m.nparts)
            todo += [(k, p) for p in range(m.nparts)]
    lmax = m.lmax()

    def one(kp):
        k, p = kp
        _refs[mesh_name, k][1][p] = FR.Reference(m.layouts[p].to_dissection(Hs[k][p]), m.layouts[p].tile, lmax)
    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(one, todo))
    return {k: _refs[mesh_name, k][1] for k in matrices}


def reference(mesh_name, matrix, H_parts=None):
    return references(mesh_name, [matrix], None if H_parts is None else {matrix: H_parts})[matrix]


def kappa(mesh_name, matrix):
    return max(float(np.linalg.cond(H)) for H in mesh(mesh_name).oracle_H(matrix))
