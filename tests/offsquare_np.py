"""Case builders of tests/test_gpu_offsquare.py: grids with nx != ny that sit on the stage
kernel's interior-tile predicate (pyrmt_amd/csrc/momentum.hip, k_mom_stage) and one cell
below it, random fields on them, the three-level level set that makes the smoothed Heaviside
exact, and a NumPy restatement of the two tile predicates (interior / pure fluid).

Plain NumPy, no GPU.
"""
import functools

import numpy as np

# stage tiles of k_mom_stage: 64 x 16 output cells.  Tile column t >= 1 is interior iff
# nx >= 64 t + 69, tile row r >= 1 iff ny >= 16 r + 21 (i0 - 3 >= 2, i0 + 67 <= nx - 2).
TX, TY = 64, 16

# (ny, nx)
SHAPES = [
    (37, 133),   # exactly one interior tile
    (36, 132),   # one cell short in both axes: none
    (53, 197),   # 2 x 2 interior tiles
    (69, 261),   # 3 x 3; the last tile column is 5 cells wide
    (68, 260),   # last interior row and column lost
    (69, 256),   # nx % 64 == 0
    (261, 69),   # transposed: no interior tile in x, many tile rows
    (5, 131),    # every row within reach of a one-sided stencil
    (131, 5),    # every column
]
SPACINGS = ["aniso", "iso"]   # dx != dy (SQ = false kernels) / dx == dy (SQ = true)


def sid(shape):
    return "%dx%d" % shape


def spacing(shape, kind):
    ny, nx = shape
    dx = 1.0 / (nx - 1)
    return (dx, 0.7 / (ny - 1)) if kind == "aniso" else (dx, dx)


@functools.lru_cache(maxsize=None)
def fields(shape, kind):
    """The inputs of every case: u, v = 0.1 N(0,1), p = N(0,1), X1 = X + 1e-3 N, X2 = Y + 1e-3 N from
    default_rng(ny * 7 + nx), X = i dx, Y = j dy; further planes (q, s1..s3, H, rho, f1, f2)
    for the operators that take more inputs.  Shared between tests: never written to."""
    ny, nx = shape
    dx, dy = spacing(shape, kind)
    rng = np.random.default_rng(ny * 7 + nx)
    X, Y = np.meshgrid(np.arange(nx) * dx, np.arange(ny) * dy)
    f = dict(dx=dx, dy=dy, X=X, Y=Y)
    f["u"] = rng.standard_normal((ny, nx)) * 0.1
    f["v"] = rng.standard_normal((ny, nx)) * 0.1
    f["p"] = rng.standard_normal((ny, nx))
    f["X1"] = X + 1e-3 * rng.standard_normal((ny, nx))
    f["X2"] = Y + 1e-3 * rng.standard_normal((ny, nx))
    for k in ("q", "s1", "s2", "s3", "f1", "f2"):
        f[k] = rng.standard_normal((ny, nx))
    f["H"] = rng.uniform(0.0, 1.0, (ny, nx))
    f["rho"] = rng.uniform(1.0, 2.0, (ny, nx))
    Lx, Ly = (nx - 1) * dx, (ny - 1) * dy
    # a disc level set for the operators that only branch on phi (sqrt is correctly rounded)
    f["phi"] = np.sqrt((X - 0.5 * Lx) ** 2 + (Y - 0.4 * Ly) ** 2) - 0.3 * min(Lx, Ly)
    # 500 query points from [-0.1, L + 0.1] per axis, then the four corners of that box: on
    # the long axis of a thin grid the random draws alone can miss the clamps
    f["xq"] = np.append(rng.uniform(-0.1, Lx + 0.1, 500), [-0.1, Lx + 0.1, -0.1, Lx + 0.1])
    f["yq"] = np.append(rng.uniform(-0.1, Ly + 0.1, 500), [-0.1, -0.1, Ly + 0.1, Ly + 0.1])
    for a in f.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return f


# ── the three-level level set ─────────────────────────────────────────────────────
def three_level_phi(shape, block):
    """phi = -1 on rows [j0, j1) x columns [i0, i1), exactly 0.0 on the one-cell ring around
    it (corners included, clipped at the grid edge), +1 elsewhere.  For any w_t < 1 the smoothed
    Heaviside of it is exactly {0, 0.5, 1}: the clamps decide +-1 and sin(0) = 0."""
    ny, nx = shape
    j0, j1, i0, i1 = block
    assert 0 <= j0 < j1 <= ny and 0 <= i0 < i1 <= nx, (shape, block)
    phi = np.ones((ny, nx))
    phi[max(j0 - 1, 0):min(j1 + 1, ny), max(i0 - 1, 0):min(i1 + 1, nx)] = 0.0
    phi[j0:j1, i0:i1] = -1.0
    return phi


# Blocks per shape, as rows [j0, j1) x columns [i0, i1):
#   far      -- inside tile (0, 0): every interior tile and its +2 halo stay phi = 1;
#   straddle -- across a corner of an interior tile where the shape has one, reaching into
#               three neighbours, placed so that over the shapes the neighbours are edge tiles
#               of every kind (default: the upper right corner of tile (1, 1), rows 16..31,
#               columns 64..127); on (261, 69) across the tile-column edge at 64;
#   cover    -- a whole tile plus its 2-cell halo solid: tile (2, 2) of (69, 261), tile (5, 0)
#               of (261, 69) (against the west wall);
#   graze_x, graze_y -- the ring ends in the column / row next to tile (1, 1) (and, on
#               (69, 261), to the tile on the block's other side): the tile's own cells are all
#               phi = 1 and the only non-fluid values it reads are in its +1 halo, so a pure-fluid
#               flag that looked one cell too few would go wrong here; tile (1, 1) is interior
#               on (69, 261) and an edge tile on (36, 132);
#   thin     -- the one block of the 5-wide grids.
_FAR, _STR = (3, 9, 4, 20), (26, 33, 118, 130)
BLOCKS = {
    (37, 133): {"far": _FAR, "straddle": _STR},
    (36, 132): {"far": _FAR, "straddle": _STR, "graze_x": (20, 28, 40, 63),
                "graze_y": (5, 15, 80, 110)},
    (53, 197): {"far": _FAR, "straddle": (40, 50, 50, 70)},      # tiles W, NW, N
    (69, 261): {"far": _FAR, "straddle": _STR, "cover": (29, 51, 125, 195),
                "graze_x": (20, 28, 129, 191), "graze_y": (33, 47, 80, 110)},
    (68, 260): {"far": _FAR, "straddle": (10, 20, 100, 140)},    # two S tiles
    (69, 256): {"far": _FAR, "straddle": (10, 20, 185, 200)},    # tiles S, SE, E
    (261, 69): {"far": _FAR, "straddle": (26, 33, 58, 67), "cover": (77, 99, 0, 67)},
    (5, 131): {"thin": (2, 3, 50, 80)},
    (131, 5): {"thin": (50, 80, 2, 3)},
}
SHAPE_BLOCKS = [(s, b) for s in SHAPES for b in BLOCKS[s]]


# ── the two tile predicates, restated ─────────────────────────────────────────────
def tile_classes(phi, thr):
    """One record per stage tile of a whole-grid momentum step (row window [0, ny)):
    (interior, sides, state, straddles).
      interior -- k_mom_stage's test: the tile's 3-cell halo inside [2, n - 2) on both axes;
      sides    -- for an edge tile, which of its sides fail that test ("S", "N", "W", "E");
      state    -- "fluid": every phi of rows [j0 - 2, j0 + 18) x columns [i0 - 2, i0 + 66)
                  inside the grid exceeds thr (k_fluid_rows / k_fluid_win: the tile takes the
                  pure-fluid shortcut); "solid": that region is all phi < 0; "mixed" else;
      straddles -- the tile's own cells hold both phi = -1 and phi = +1 (a block edge)."""
    ny, nx = phi.shape
    out = []
    for j0 in range(0, ny, TY):
        for i0 in range(0, nx, TX):
            sides = ("S" if j0 - 3 < 2 else "") + ("N" if j0 + TY + 3 > ny - 2 else "") + \
                    ("W" if i0 - 3 < 2 else "") + ("E" if i0 + TX + 3 > nx - 2 else "")
            reg = phi[max(j0 - 2, 0):min(j0 + TY + 2, ny), max(i0 - 2, 0):min(i0 + TX + 2, nx)]
            state = "fluid" if (reg > thr).all() else "solid" if (reg < 0).all() else "mixed"
            own = phi[j0:j0 + TY, i0:i0 + TX]
            out.append((sides == "", sides, state, bool((own < 0).any() and (own > 0).any())))
    return out


def interior_tile_count(shape):
    ny, nx = shape
    return max((nx - 69) // TX, 0) * max((ny - 21) // TY, 0)
