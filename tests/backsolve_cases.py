"""The cases of tests/test_gpu_backsolve_forms.py and what the host-only planner says about them (no GPU): which instantiation of
the back-solve kernels (dot_amd/csrc/k_backsolve.hip) every tile of a case's job table goes to, and the rows whose unit vectors the
GPU test applies.  The forms -- their names, the longest row each takes and its rows per pass -- are read from the table the kernels
are instantiated from (dot_amd/csrc/bs_forms.hpp, through the host-only entry dotmi_plan_backsolve_forms); the forms per case are
pinned in CASES below and checked on the CPU by tests/test_backsolve_reference.py, so a change of that table that takes a form out of
the GPU test's reach, or renames one, fails there."""
import ctypes as C

import numpy as np

from dot_amd import lib as dl


def _forms():
    """per family [(name, longest row it takes, rows per pass)] in the table's order, and the two-phase kernel's (rows per pass,
    columns per chunk)"""
    L = dl.load()
    counts = np.zeros(4, dtype=np.int32)
    assert L.dotmi_plan_backsolve_forms(0, None, dl.ip(counts)) == 0
    rows = np.zeros((int(counts[0]), 6), dtype=np.int32)
    assert L.dotmi_plan_backsolve_forms(rows.shape[0], dl.ip(rows), dl.ip(counts)) == 0
    fams = [[], [], []]
    for fam, lanes, chunks, sub, rlds, longest in rows.tolist():
        name = f"wave<{chunks},{sub}>" if fam == 0 else f"tile<{lanes},{chunks},{sub}{',RLDS' if rlds else ''}>"
        fams[fam].append((name, longest, sub))
    return fams, int(counts[2]), int(counts[3])


(PACK_FORMS, NARROW_FORMS, _WIDE_ALL), _LONG_SUB, LONG_CHUNK = _forms()
# the 512-thread forms whose rows the 256-thread family holds as well take tiles only in GSDD's per-part launch (below)
WIDE_FORMS = [f for f in _WIDE_ALL if f[1] > NARROW_FORMS[-1][1]]
LONG_FORM = ("long", 1 << 30, _LONG_SUB)
ROWS_PER_PASS = dict((f[0], f[2]) for f in PACK_FORMS + NARROW_FORMS + WIDE_FORMS + [LONG_FORM])
# every instantiation the all-parts launch (launch_gemv) can reach.  backsolve_tile<512,1,32> and <512,2,16> take tiles only in GSDD's
# per-part launch (launch_gemv_part with maxTileLen > 3072), which no entry applies on its own: out of scope
ALL_FORMS = set(ROWS_PER_PASS)

# (workload, switches) -> the forms its job table must reach and the chunk counts of its two-phase tiles
_BIG = {"wave<1,32>", "wave<2,16>", "tile<256,1,32>", "tile<256,2,16>", "tile<256,3,8>", "tile<256,5,8>", "tile<256,6,8,RLDS>",
        "tile<512,4,8>", "long"}
CASES = {
    "24x8x8": ("synbar:24x8x8:1", {}, _BIG, {2}),
    "24x8x8-rows64": ("synbar:24x8x8:1", {"DOTMI_TILE_ROWS": "64"}, _BIG, {2}),
    "24x8x8-rows8": ("synbar:24x8x8:1", {"DOTMI_TILE_ROWS": "8"}, _BIG, {2}),
    "24x8x8-nopacks": ("synbar:24x8x8:1", {"DOTMI_WAVE_PACKS": "0"}, _BIG - {"wave<1,32>", "wave<2,16>"}, {2}),
    "24x8x8-long8": ("synbar:24x8x8:1", {"DOTMI_TILE_ROWS_LONG": "8"}, _BIG, {2}),
    "26x9x9": ("synbar:26x9x9:1", {}, {"wave<1,32>", "wave<2,16>", "tile<256,1,32>", "tile<256,2,16>", "tile<256,5,8>", "tile<512,4,8>",
                                      "tile<512,5,8>", "long"}, {3}),
    "16x5x5-4parts": ("synbar:16x5x5:4", {}, {"wave<1,32>", "wave<2,16>", "tile<256,2,16>"}, set()),
    "40x10x10-256parts": ("synbar:40x10x10:256", {}, {"wave<1,32>", "wave<2,16>"}, set()),
}
MAX_APPLIES = 256
TILES_PER_FORM = 4


class Plan:
    """the job table of a case: tiles[:, 6] = part, first row, rows, first column, tile index in the part, job; form[t] and the
    layout (nodes, nmax, pos, verts of dot_amd.sharding.plan_layout)"""

    def __init__(self, case):
        from dot_amd.workloads import load_workload
        from tests.test_host_logic import _plan_bs_tiles
        name, env, _, _ = CASES[case]
        self.case = case
        self.sc, self.ep, self.nparts = sc, ep, n = load_workload(name)
        # the case's environment: form 0 of the block solve and the case's own switches
        tiles, counts, self.nodes, self.nmax, self.pos, _ = _plan_bs_tiles(name, dict(env, DOTMI_TWO_LEVEL="0"))
        self.verts = [np.unique(np.asarray(sc.T)[np.asarray(ep) == p]).astype(np.int32) for p in range(n)]
        assert counts["nmax"] == self.nmax
        self.tiles = tiles
        self.n_wide, self.n_narrow, self.n_packs = counts["n_wide"], counts["n_narrow"], counts["n_packs"]
        part, r0, rows, cb, idx, job = tiles.T
        self.len = r0 + rows - cb                       # the tile's longest row, first column to diagonal
        self.form = np.array([self._form(int(l), int(j)) for l, j in zip(self.len, job)])
        self.chunks = np.where(job < 0, (((self.len + 15) & ~15) + LONG_CHUNK - 1) // LONG_CHUNK, 0)
        # row -> (local vertex, component) per part
        self.row_vertex = []
        for p in range(n):
            rv = np.full(self.nmax, -1, dtype=np.int64)
            for d in range(3):
                rv[self.pos[p] + d] = 3 * np.arange(self.pos[p].size) + d
            self.row_vertex.append(rv)

    def _form(self, ln, job):
        if job < 0:
            assert ln > WIDE_FORMS[-1][1]
            return LONG_FORM[0]
        if ln > NARROW_FORMS[-1][1]:
            table = WIDE_FORMS
        elif self.n_packs and job >= self.n_narrow:
            table = PACK_FORMS
        else:
            table = NARROW_FORMS
        for name, longest, _ in table:
            if ln <= longest:
                return name
        raise AssertionError((ln, job))

    def global_dof(self, part, row):
        """the scalar dof 3 v + d stored in `row` of `part`, -1 on padding"""
        k = self.row_vertex[part][row]
        return -1 if k < 0 else 3 * int(self.verts[part][k // 3]) + int(k % 3)

    def tile_of(self, part, row):
        """index into tiles of the tile that holds `row` of `part`"""
        t = np.flatnonzero((self.tiles[:, 0] == part) & (self.tiles[:, 1] <= row) & (row < self.tiles[:, 1] + self.tiles[:, 2]))
        return int(t[0]) if t.size else -1

    def locate(self, dof):
        """where the job table puts a global scalar dof: [(part, tile index, form, row)]"""
        out = []
        v, d = divmod(int(dof), 3)
        for p in range(self.nparts):
            k = np.searchsorted(self.verts[p], v)
            if k < self.verts[p].size and self.verts[p][k] == v:
                row = int(self.pos[p][k]) + d
                t = self.tile_of(p, row)
                out.append((p, int(self.tiles[t, 4]), str(self.form[t]), row) if t >= 0 else (p, -1, "no tile", row))
        return out

    def root_separator_vertices(self):
        """global vertices that sit in the root separator of some subdomain (node 0 of the layout, when it is split at all)"""
        off, size, a, c, offS, sizeS = (int(x) for x in self.nodes[0])
        if a < 0:
            return np.zeros(0, dtype=np.int64)
        vs = [self.verts[p][(self.pos[p] >= offS) & (self.pos[p] < offS + sizeS)] for p in range(self.nparts)]
        return np.unique(np.concatenate(vs)).astype(np.int64)

    def sweep_rows(self):
        """The unit vectors of the case: (global dof, part, tile, row, why), at most MAX_APPLIES, distinct dofs.
        Per form TILES_PER_FORM tiles -- the one with the longest row, the one with the shortest, one that starts inside a 64-row
        block (a first tile that ends at the next block) when there is one, the one with the fewest rows, then evenly spaced by row
        length; per tile the first and the last live row and the two rows on either side of every pass boundary of its form; per
        two-phase tile one row whose diagonal lies in each 4096-column chunk of the tile's columns.  When that is more than the cap,
        the rows are kept in this order: first / last rows and chunk rows of every tile, then the pass boundaries of all tiles in
        turn (a tile's first boundary, its last, the ones between) -- so every chosen tile keeps its edges and loses inner
        boundaries only."""
        fixed = np.asarray(self.sc.fixed, dtype=bool)
        part, r0, rows, cb, idx, job = self.tiles.T
        must, rounds, taken = [], [], set()
        for form in sorted(set(self.form)):
            ts = np.flatnonzero(self.form == form)
            ts = ts[np.argsort(self.len[ts], kind="stable")]
            pick = [ts[-1], ts[0]]
            inner = [t for t in ts if r0[t] % 64 != 0]
            if inner:
                pick.append(inner[-1])
            pick.append(ts[np.argmin(rows[ts])])
            pick += [ts[(k * (ts.size - 1)) // 5] for k in range(1, 5)] + list(ts)
            chosen = []
            sub = ROWS_PER_PASS[form]
            for t in (int(t) for t in pick):
                if t in chosen or len(chosen) >= TILES_PER_FORM:
                    continue
                p, a, b = int(part[t]), int(r0[t]), int(r0[t] + rows[t])
                # (a fixed vertex has no right-hand side, and a dof is applied once: the tile's first / last row of a free vertex
                # no other tile has taken; a tile without one is passed over)
                free = [x for x in range(a, b) if not fixed[self.global_dof(p, x) // 3] and self.global_dof(p, x) not in taken]
                if not free:
                    continue
                chosen.append(t)
                taken.update(self.global_dof(p, x) for x in (free[0], free[-1]))
                must += [(p, t, free[0], "first row"), (p, t, free[-1], "last row")]
                bnd = list(range(a + sub, b, sub))
                order = bnd[:1] + bnd[-1:] + bnd[1:-1]
                for k, x in enumerate(dict.fromkeys(order)):
                    while len(rounds) <= k:
                        rounds.append([])
                    rounds[k] += [(p, t, x - 1, "last row of a pass"), (p, t, x, "first row of a pass")]
        for t in np.flatnonzero(job < 0):
            p = int(part[t])
            live = np.flatnonzero(self.row_vertex[p] >= 0)
            for c in range(int(self.chunks[t])):
                lo = int(cb[t]) + c * LONG_CHUNK
                inside = live[(live >= lo) & (live < min(lo + LONG_CHUNK, int(r0[t] + rows[t])))]
                inside = [r for r in inside if not fixed[self.global_dof(p, int(r)) // 3]]
                if inside:   # (listed under the tile that holds the row itself)
                    row = int(inside[len(inside) // 2])
                    must.append((p, self.tile_of(p, row), row, f"diagonal in column chunk {c} of two-phase tile {int(idx[t])}"))
        out, seen = [], set()
        for p, t, row, why in must + [x for rnd in rounds for x in rnd]:
            dof = self.global_dof(p, row)
            if dof < 0 or fixed[dof // 3] or dof in seen or len(out) >= MAX_APPLIES:
                continue
            seen.add(dof)
            out.append((dof, p, int(t), int(row), why))
        wanted = len({self.global_dof(p, row) for p, t, row, why in must + [x for rnd in rounds for x in rnd]} - {-1})
        return out, wanted
