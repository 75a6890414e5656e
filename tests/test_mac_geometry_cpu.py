"""Geometry cases of the config-5 MAC loop (rmt_mac_sim_step) and the conditions that make a
device-against-oracle comparison on them meaningful.  No GPU: the oracle alone.

The loop decides per disc where it works: mac_cover grows, clamps and rounds the support
boxes to SL tiles (mac_disc_update); mac_stress_predict launches the stress on the boxes and
the predictor adds a zero force away from them; mac_diag_rows gives the diagnostics' row
range; mac_sched switches box mode and the contact shortcut by disc_phi(0, 0).  The
cases below put discs where those decisions change: at and across walls, K = 1, 5 and 8, N not
a multiple of 4 or 64, a box wider than one 256-column block, the origin near and inside a
disc.  tests/test_gpu_mac_geometry.py runs the device loop on the same table.

Each case has to be a run the comparison can hold on: no folded map (a disc's band within
about two rows of the lid folds in the reference itself within six steps), every disc keeping
cells, and no phi so close to zero that the ~1e-13 differences between two DCT-II
implementations could move a cell across phi <= 0 (which moves a centroid by ~1e-4).  The bounds
here are caps chosen before any device run, not measurements.
"""
import functools
import warnings

import numpy as np
import pytest

_G3 = (0.2, 0.5, 0.8)
EIGHT = [(0.11 + 0.004 * k, _G3[k % 3] + 0.003 * k, _G3[k // 3] - 0.002 * k) for k in range(8)]

# name -> (N, specs (R, cx, cy), MacMultiDisc keywords, steps)
CASES = {
    # boxes clamped at column 1 / row 1 / column N-2; N no multiple of 4 or 64
    "walls": (50, [(0.1, 0.131, 0.507), (0.08, 0.883, 0.117), (0.09, 0.871, 0.613)], {}, 6),
    # a disc cut by the left wall: its support starts at column 0
    "cut": (52, [(0.1, 0.073, 0.41), (0.1, 0.6, 0.3)], {}, 6),
    # K = MAC_MAXD, 28 contact pairs, overlapping boxes, cells with both phi < eps
    "eight": (96, EIGHT, {}, 6),
    # K = 5: MS_BLOCKS / K truncates
    "five": (80, [EIGHT[k] for k in (0, 1, 3, 4, 7)], {}, 6),
    # K = 1, no pair, odd N
    "one": (33, [(0.2, 0.45, 0.55)], {}, 6),
    # 0 < disc_phi(0, 0) < eps: box mode on, contact shortcut off (stress on the full grid)
    "near_origin": (32, [(0.1, 0.13, 0.13), (0.12, 0.6, 0.6)], {}, 6),
    # disc_phi(0, 0) < 0: box mode off although mac_boxes = 1.  One step: see FOLDS
    "origin_inside": (40, [(0.15, 0.1, 0.093), (0.1, 0.6, 0.5)], {}, 1),
    # a box about 275 columns wide: two 256-column blocks per row
    "wide": (320, [(0.42, 0.503, 0.498)], {}, 3),
    # eta = 0: the contact loop is skipped while both phi < eps
    "eta0": (48, [(0.1, 0.35, 0.5), (0.1, 0.6, 0.5)], {"eta": 0.0}, 6),
    # other constants (dt still the advective bound 0.3 dx / U, as with the defaults)
    "props": (40, [(0.1, 0.35, 0.5), (0.12, 0.65, 0.55)],
              {"rho": 1.7, "mu_f": 0.02, "mu_s": 0.5}, 6),
    # dt from another branch of the min: the viscous bound 0.2 dx^2 rho / mu_f
    "visc": (40, [(0.1, 0.35, 0.5), (0.12, 0.65, 0.55)],
             {"rho": 1.7, "mu_f": 0.05, "mu_s": 0.5}, 6),
    # smaller than an SL tile and a 9 x 9 fit window
    "small": (9, [(0.25, 0.45, 0.5)], {}, 6),
    # discs that travel: the run starts from a vortex (INITIAL_FLOW), so the supports leave
    # the SL tiles of their last boxes.  From rest nothing moves a cell within 40 steps and
    # the growth G of the boxes is never needed.
    "swirl": (50, [(0.1, 0.3, 0.507), (0.09, 0.663, 0.371), (0.08, 0.553, 0.723)], {}, 12),
}
# amplitude A of the initial stream function psi = A sin^2(pi x) sin^2(pi y) on the grid nodes
# (max |u| = pi A); the other cases start from rest
INITIAL_FLOW = {"swirl": 0.75 / np.pi}


def initial_flow(name):
    """(u, v) a case starts from, or None: differences of psi along the faces, so the field is
    discretely divergence-free and zero on the wall-normal faces."""
    if name not in INITIAL_FLOW:
        return None
    N = CASES[name][0]
    g = np.sin(np.pi * np.arange(N + 1) / N) ** 2
    g[0] = g[-1] = 0.0
    psi = INITIAL_FLOW[name] * g[:, None] * g[None, :]      # psi[j, i] at node (x_i, y_j)
    u = (psi[1:, :] - psi[:-1, :]) * N
    v = -(psi[:, 1:] - psi[:, :-1]) * N
    return u, v


def covered(box, N, G):
    """The cells mac_disc_update's passes cover for a support box (mac_cover's cb, held to
    it by test_covered_restates_mac_cover): grown by G, clamped, rounded out to whole 4 x 64
    SL tiles ((j0, j1, i0, i1), half-open)."""
    cb = [max(0, box[0] - G), min(N, box[1] + 1 + G), max(0, box[2] - G), min(N, box[3] + 1 + G)]
    cb[0] -= cb[0] % 4; cb[1] = min(N, (cb[1] + 3) // 4 * 4)
    cb[2] -= cb[2] % 64; cb[3] = min(N, (cb[3] + 63) // 64 * 64)
    return cb
# Cases the reference itself folds on, whatever the placement.  With the origin inside a disc
# every cell the map leaves at zero has phi = disc_phi(0, 0) < 0 and counts as solid, so the
# stress sees the jump from the map to zero at the support's edge: J = -14.4 in the first step
# here (only a disc covering the whole grid would avoid it, and would have no box to get wrong).
# The loop records that step, flags it and stops; the comparison is of that one step.
FOLDS = {"origin_inside"}
# the empty-map run: the first disc holds no cell centre
EMPTY = (32, [(0.004, 0.5, 0.5), (0.12, 0.3, 0.6)])


def origin_phi(spec):
    """disc_phi(0, 0): what mac_sched switches box mode and the contact shortcut on."""
    R, cx, cy = spec
    return np.sqrt(cx * cx + cy * cy) - R


def support_box(X1, X2):
    """(row min, row max, col min, col max) of the cells where the map is not zero."""
    j, i = np.nonzero((X1 != 0) | (X2 != 0))
    return int(j.min()), int(j.max()), int(i.min()), int(i.max())


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle's run of a case, computed once per process and shared (read-only) by every
    test: the step records, the initial and final maps, and what the conditions read."""
    from oracle import mac_oracle as MO
    N, specs, kw, steps = CASES[name]
    sim = MO.MacMultiDisc(N, specs=specs, **kw)
    if name in INITIAL_FLOW:
        sim.u, sim.v = initial_flow(name)
    out = dict(sim=sim, X1_0=[r[0].copy() for r in sim.refs],
               box0=[support_box(*r) for r in sim.refs], recs=[], min_abs_phi=np.inf,
               min_cells=N * N, both_eps=0, boxes=[])
    for _ in range(steps):
        out["recs"].append(sim.step())
        out["min_abs_phi"] = min(out["min_abs_phi"], min(np.abs(q).min() for q in sim.phis))
        out["min_cells"] = min(out["min_cells"], min(int((q <= 0).sum()) for q in sim.phis))
        for a in range(len(specs)):
            for b in range(a + 1, len(specs)):
                both = (sim.phis[a] < sim.eps) & (sim.phis[b] < sim.eps)
                out["both_eps"] = max(out["both_eps"], int(both.sum()))
        out["boxes"].append([support_box(*r) for r in sim.refs])
    for a in [sim.u, sim.v] + [x for r in sim.refs for x in r] + out["X1_0"]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_a_healthy_run(name):
    N, specs, kw, steps = CASES[name]
    r = oracle_run(name)
    assert len(r["recs"]) == steps
    for rec in r["recs"]:
        assert np.isfinite(rec["cx"]).all() and np.isfinite(rec["cy"]).all()
        if name in FOLDS:
            assert steps == 1 and rec["minJ"] < -1.0 and rec["maxJ"] <= 1.5
        else:
            assert 0.9 <= rec["minJ"] <= rec["maxJ"] <= 1.5, (rec["minJ"], rec["maxJ"])
    assert np.isfinite(r["sim"].u).all() and np.isfinite(r["sim"].v).all()
    assert r["min_cells"] > 0
    assert r["min_abs_phi"] >= 1e-9, r["min_abs_phi"]


def test_walls_boxes_are_clamped():
    """The support boxes stop short of the walls by less than the growth G = layers + 6, so
    the grown box is clamped at the left, bottom and right walls (and N is no multiple of 4)."""
    N = CASES["walls"][0]
    r = oracle_run("walls")
    b = r["box0"]
    assert N % 4 and N % 64
    assert b[0][2] == 1 and b[1][0] == 1 and b[1][3] == N - 2 and b[2][3] == N - 2
    for boxes in r["boxes"]:
        assert all(x[0] >= 1 and x[2] >= 1 and x[3] <= N - 2 for x in boxes)


def test_swirl_supports_leave_their_tiles():
    """In `swirl` some support leaves the whole SL tiles of its previous box (G = 0), so the
    boxes' growth is needed; one step never moves a support by more than one cell, far below
    G = layers + 6."""
    N = CASES["swirl"][0]
    r = oracle_run("swirl")
    seq = [r["box0"]] + r["boxes"]
    left, grow = 0, 0
    for old, new in zip(seq[:-1], seq[1:]):
        for o, n in zip(old, new):
            cb = covered(o, N, 0)
            left += n[0] < cb[0] or n[1] >= cb[1] or n[2] < cb[2] or n[3] >= cb[3]
            grow = max(grow, o[0] - n[0], n[1] - o[1], o[2] - n[2], n[3] - o[3])
    assert left >= 1 and grow == 1, (left, grow)
    assert 0.7 < max(np.abs(a).max() for a in initial_flow("swirl")) <= 0.75


LAYERS = 3      # the loop's extrapolation layers (mac_params; the oracle's MacMultiDisc)


def cover_edge_inputs():
    """(N, G, box) beyond the cases' boxes: an empty box (k_box_reduce's), a box touching all
    four walls, and per N boxes whose grown upper column i1 + 1 + G lands exactly on a
    multiple of 64, on N and on N - 1 (where a grid of that size has such a column)."""
    out = [(32, 9, (2 ** 31 - 1, -1, 2 ** 31 - 1, -1)), (50, 9, (0, 49, 0, 49))]
    for N in (9, 33, 50, 64, 320):
        out += [(N, 9, (2 ** 31 - 1, -1, 2 ** 31 - 1, -1)), (N, 9, (0, N - 1, 0, N - 1))]
        for G in (3, 9):
            for top in sorted({64, 128, 256, N - 1, N}):
                i1 = top - 1 - G
                if 0 <= i1 < N:
                    i0 = max(0, i1 - 5)
                    out += [(N, G, (i0, i1, i0, i1)), (N, G, (1, min(N - 1, 3), 0, i1))]
    return out


def test_covered_restates_mac_cover(tmp_path):
    """covered() above against mac_cover of pyrmt_amd/csrc/mac_cover.hpp (compiled for the
    host: tools/mac_cover_check.hip), on every support box of every case and the edge inputs;
    the no-op test's rows and words against their definition: rows [cb0 - 1, cb1 + 1) within
    the grid, the 64-column words of columns [cb2 - 1, cb3 + 1) within it, and one row, one
    word and no cell for an empty box."""
    import os
    import subprocess
    from conftest import ROOT
    inputs = cover_edge_inputs()
    for name in sorted(CASES):
        r = oracle_run(name)
        for boxes in [r["box0"]] + r["boxes"]:
            inputs += [(CASES[name][0], LAYERS + 6, b) for b in boxes]
    exe = str(tmp_path / "mac_cover_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe,
                    os.path.join(ROOT, "tools", "mac_cover_check.hip")], check=True)
    text = "".join("%d %d %d %d %d %d\n" % ((N, G) + tuple(b)) for N, G, b in inputs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True)
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(inputs) >= 100
    tops = set()
    for (N, G, b), got in zip(inputs, rows):
        cb, none_rows, none_cols, empty = got[:4], got[4:6], got[6:8], got[8]
        assert empty == (b[1] < b[0]), (N, G, b)
        if empty:
            assert (cb, none_rows, none_cols) == ([0, 0, 0, 0], [0, 1], [0, 1]), (N, G, b)
            continue
        assert cb == covered(b, N, G), (N, G, b, cb)
        assert none_rows == [max(0, cb[0] - 1), min(N, cb[1] + 1)], (N, G, b, none_rows)
        cols = [i for i in range(cb[2] - 1, cb[3] + 1) if 0 <= i < N]
        assert none_cols == [cols[0] // 64, cols[-1] // 64 + 1], (N, G, b, none_cols)
        tops.add((N, b[3] + 1 + G))
    # the edge inputs reach what they are for
    for N in (9, 33, 50, 64, 320):
        assert {(N, N - 1), (N, N)} <= tops
    assert {(320, 64), (320, 128), (320, 256), (64, 64)} <= tops


def test_cut_support_has_column_0():
    r = oracle_run("cut")
    assert r["box0"][0][2] == 0
    assert all(boxes[0][2] == 0 for boxes in r["boxes"])
    assert origin_phi(CASES["cut"][1][0]) >= 3.0 / CASES["cut"][0]   # contact shortcut stays on


def test_wide_box_needs_two_blocks():
    b = oracle_run("wide")["box0"][0]
    assert 256 < b[3] - b[2] + 1 + 2 * 9 <= 512     # the box grown by G = 9: nbx = 2
    assert b[3] - b[2] + 1 > 256                    # and the support alone already


def test_eight_and_five_reach_contact():
    assert len(CASES["eight"][1]) == 8 and len(CASES["five"][1]) == 5
    assert oracle_run("eight")["both_eps"] >= 1
    assert oracle_run("five")["both_eps"] >= 1
    # overlapping boxes: two initial support boxes share a cell
    b = oracle_run("eight")["box0"]
    assert any(b[p][0] <= b[q][1] and b[q][0] <= b[p][1] and b[p][2] <= b[q][3] and
               b[q][2] <= b[p][3] for p in range(8) for q in range(p + 1, 8))


def test_eta0_has_cells_the_contact_loop_would_take():
    assert oracle_run("eta0")["both_eps"] >= 1


def test_origin_cases():
    N, specs, _, _ = CASES["near_origin"]
    p0 = origin_phi(specs[0])
    assert 0.0 < p0 < 3.0 / N                       # box mode on, contact = 0
    assert origin_phi(specs[1]) >= 3.0 / N
    N, specs, _, _ = CASES["origin_inside"]
    assert origin_phi(specs[0]) < -1e-3             # box mode off
    assert origin_phi(specs[1]) >= 3.0 / N
    # every other case: box mode on with the contact shortcut
    for name, (N, specs, _, _) in CASES.items():
        if name not in ("near_origin", "origin_inside"):
            assert all(origin_phi(s) >= 3.0 / N for s in specs), name


def test_dt_branches():
    """`props` changes the viscous and elastic bounds but dt stays the advective one (branch
    0, as with the default constants); `visc` takes the viscous bound (branch 1)."""
    def branches(N, U=1.0, mu_s=0.3, mu_f=0.01, rho=1.0):
        dx = 1.0 / N
        return (0.3 * dx / U, 0.2 * dx * dx / (mu_f / rho),
                0.3 * dx / (np.sqrt(mu_s / rho) + 1e-9))
    assert int(np.argmin(branches(40))) == 0
    for name, which in (("props", 0), ("visc", 1)):
        N, _, kw, _ = CASES[name]
        d = branches(N, **kw)
        assert int(np.argmin(d)) == which
        assert oracle_run(name)["sim"].dt == min(d)


def test_t_end_gives_four_records_in_the_oracle():
    """t_end = 3.5 dt on `one`: three full steps and one of t_end - t, after which t >= t_end
    (t + (t_end - t) does not fall short of t_end here, which would add a fifth record)."""
    from oracle import mac_oracle as MO
    N, specs, kw, _ = CASES["one"]
    sim = MO.MacMultiDisc(N, specs=specs, **kw)
    t_end = 3.5 * sim.dt
    recs = []
    while sim.t < t_end and len(recs) < 8:
        recs.append(sim.step(t_end))
    assert [r["dt"] == sim.dt for r in recs] == [True, True, True, False]
    assert 0 < recs[3]["dt"] < sim.dt and sim.t >= t_end


def test_empty_map_in_the_oracle():
    """The first disc of EMPTY holds no cell centre: its centroid is NaN after one step and
    the second disc moves as it does alone."""
    from oracle import mac_oracle as MO
    N, specs = EMPTY
    assert min(origin_phi(s) for s in specs) >= 3.0 / N     # box mode on, with the shortcut
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # mean of an empty selection
        sim = MO.MacMultiDisc(N, specs=specs)
        assert not (sim.refs[0][0] != 0).any() and not (sim.refs[0][1] != 0).any()
        rec = sim.step()
    assert np.isnan(rec["cx"][0]) and np.isnan(rec["cy"][0])
    alone = MO.MacMultiDisc(N, specs=specs[1:])
    ra = alone.step()
    assert rec["cx"][1] == ra["cx"][0] and rec["cy"][1] == ra["cy"][0]
    np.testing.assert_array_equal(sim.refs[1][0], alone.refs[0][0])
    np.testing.assert_array_equal(sim.u, alone.u)
