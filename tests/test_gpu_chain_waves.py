"""The extrapolation chain at 8 and at 16 waves per part (option chain_waves, extrap_chain.hip).

The wave count changes how many waves share a part's fits (round robin l % W), how many of a
fit's tail terms wait in registers (8 waves: all of them, 16: the first 24, the rest folded
from LDS after the critical value arrives) and nothing else: every fit adds the same terms in
the same order.  So X1 and X2 after an extrapolation are compared BITWISE (uint64 views)
  * at 8 waves against 16 waves,
  * at 8 waves against the oracle's serial raster-order result,
  * at 16 waves against the oracle (the bar of test_gpu_parity.py / test_gpu_configs.py),
and every call must have run the chain itself: path 0 (no fallback to the row-ticket sweep; an
abort is an error of the call), on a context of its own whose option the test sets.

What a case has to contain is established on the CPU first, by a restatement of the chain's
record layout (_chain_model: targets, acceptance, chain order, parts, the critical term kc of
every fit and its tail chunks) and asserted before anything runs on the GPU:
  parts      parts with fewer fits than waves, an empty part, cross-part sources
  rejection  a rejected target (k_ex_fix re-fits; the waves' sequences skip its record)
  tails      a fit whose critical term is its last (h0 >= nch), one with a single tail chunk,
             one whose tail is longer than the 3 chunks 16 waves keep in registers, and the
             longest tail a record can have (10 chunks: 80 terms, the critical one first)
  ring       one part with more than CH_R = 2048 fits (slot reuse, the watermark wait)
  fused      the whole step at N = 128, 3 steps, every plane and diagnostic, also through the
             slab path at one rank
"""
import math

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

CH_R, CH_MAXP, CH_TVS = 2048, 8, 88   # extrap.hpp


# ------------------------------------------------------------------ the CPU model ----
def _dilate(k):
    p = np.pad(k, 1)
    out = np.zeros_like(k)
    for dj in range(3):
        for di in range(3):
            out |= p[dj:dj + k.shape[0], di:di + k.shape[1]]
    return out


def _chain_model(phi, dx, dy, ML, cols, lgroups):
    """extrap_chain.hip restated: per accepted fit its part, ordinal within the part, critical
    term kc (None: no local source), chunks nch and first tail chunk h0; per part its fit count
    (accepted or not: the ring is indexed by ordinal); the rejected targets; the number of
    cross-part sources."""
    ny, nx = phi.shape
    known0 = phi < 0
    r = 4 * math.sqrt(dx * dx + dy * dy)
    r2 = r * r
    interior = np.zeros_like(known0)
    interior[1:-1, 1:-1] = True
    known = known0.copy()
    fid = -np.ones((ny, nx), dtype=np.int64)
    fits, accepted, window = [], [], []
    for L in range(ML):
        tgt = (~known) & _dilate(known) & interior
        acc = np.zeros_like(known)
        for j, i in zip(*np.nonzero(tgt)):   # raster order
            j, i = int(j), int(i)
            x0, y0 = dx * i, dy * j
            cells, A = [], np.zeros(6)
            for q in range(81):
                jj, ii = j - 4 + q // 9, i - 4 + q % 9
                if not (0 <= jj < ny and 0 <= ii < nx):
                    continue
                xi, yi = dx * ii, dy * jj
                d2 = (xi - x0) ** 2 + (yi - y0) ** 2
                if d2 > r2 or not (known[jj, ii] or acc[jj, ii]):
                    continue   # (acc holds earlier raster positions only)
                w = math.exp(-d2 / r2)
                A += w * np.array([1.0, xi, yi, xi * xi, xi * yi, yi * yi])
                cells.append((q, jj, ii))
            M = np.array([[A[0], A[1], A[2]], [A[1], A[3], A[4]], [A[2], A[4], A[5]]])
            det = (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1])
                   - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
                   + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))
            ok = len(cells) >= 3 and abs(det) > 1e-10
            assert not (len(cells) >= 3 and 0.5e-10 < abs(det) < 2e-10), "borderline det"
            fid[j, i] = len(fits)
            fits.append((L, j, i)); accepted.append(ok); window.append(cells)
            acc[j, i] = ok
        known = known | acc
    nf = len(fits)
    if nf == 0:
        return dict(fits=[], parts=np.zeros(CH_MAXP, int), rejected=0, far=0)
    order = sorted(range(nf), key=lambda t: (fits[t][1] + 5 * fits[t][0], fits[t][0], fits[t][2]))
    chain = np.empty(nf, dtype=np.int64)
    chain[order] = np.arange(nf)
    ncol = min(CH_MAXP, max(1, cols))
    nlg = max(1, min(lgroups if lgroups > 0 else ML, ML, CH_MAXP // ncol))
    ci = np.array([f[2] for f in fits])
    cmin, span = ci.min(), ci.max() - ci.min() + 1
    col = np.clip((ci - cmin) * ncol // span, 0, ncol - 1) if ncol > 1 else np.zeros(nf, int)
    part = col * nlg + np.array([f[0] for f in fits]) * nlg // ML
    loc = np.empty(nf, dtype=np.int64)
    count = np.zeros(CH_MAXP, dtype=np.int64)
    for t in order:
        loc[t] = count[part[t]]; count[part[t]] += 1
    out, far = [], 0
    for t in range(nf):
        if not accepted[t]:
            continue
        terms = [(q, jj, ii, known0[jj, ii]) for q, jj, ii in window[t]]
        dyn = [k for k, c in enumerate(terms) if not c[3]]
        if not dyn:
            out.append(dict(t=t, part=part[t], loc=loc[t], kc=None, nch=0, h0=0, nd=0))
            continue
        terms = terms[dyn[0]:]   # the record starts at the first dynamic cell
        n = len(terms)
        npad = (n + 7) & ~7
        assert npad <= CH_TVS
        best, kc, nd = -1, None, 0
        for k, (q, jj, ii, st) in enumerate(terms):
            if st:
                continue
            s = fid[jj, ii]
            assert s >= 0 and accepted[s] and chain[s] < chain[t]
            nd += 1
            if part[s] != part[t]:
                far += 1
            elif loc[s] > best:
                best, kc = loc[s], k
                assert loc[t] - loc[s] < CH_R // 2, "ring distance: the chain would fall back"
        out.append(dict(t=t, part=part[t], loc=loc[t], kc=kc, nch=npad >> 3,
                        h0=None if kc is None else (kc + 1) >> 3, nd=nd))
    return dict(fits=out, parts=count, rejected=nf - sum(accepted), far=far,
                nparts=ncol * nlg)


def _tails(model):
    """(number of fits whose critical term is the last, with a single tail chunk, the longest
    tail in chunks)"""
    f = [x for x in model["fits"] if x["kc"] is not None]
    last = sum(x["h0"] >= x["nch"] for x in f)
    one = sum(x["nch"] - x["h0"] == 1 for x in f)
    longest = max((x["nch"] - x["h0"] for x in f), default=0)
    return last, one, longest


# ------------------------------------------------------------------ the cases --------
def _deformed(ny, nx):
    """A deformed-disc map on ny x nx (test_gpu_parity._extrap_case's map)."""
    x = np.linspace(0.0, 1.0, nx); y = np.linspace(0.0, 1.0, ny)
    X, Y = np.meshgrid(x, y)
    X1 = X + 0.05 * np.sin(2 * np.pi * Y) * np.cos(np.pi * X)
    X2 = Y + 0.03 * np.sin(2 * np.pi * X)
    phi = np.sqrt((X1 - 0.6) ** 2 + (X2 - 0.5) ** 2) - 0.2
    solid = (phi < 0).astype(float)
    return X1 * solid, X2 * solid, phi, 1.0 / (nx - 1), 1.0 / (ny - 1), 3


def _driver33(oracle):
    """The N = 33 soft-disc driver's state after the steps of its golden trajectory (checked
    against the fixture), masked the way the step hands it to the extrapolation."""
    g = golden("soft_disc_driver33")
    s = oracle.SoftDisc(33, "lid")
    rec = [s.step(t_end=0.006) for _ in range(len(g["traj"]))]
    np.testing.assert_allclose([r["cx"] for r in rec], g["traj"][:, 1], rtol=1e-12)
    phi = s.phi_of(s.X1, s.X2)
    solid = (phi < 0).astype(float)
    return s.X1 * solid, s.X2 * solid, phi, s.dx, s.dy, s.layers


def _thin(ny=64, nx=64):
    """Solid cells too few and collinear for the fits next to them: a one-cell-wide horizontal
    bar leaves every first-layer target above and below its ends with a singular or
    near-singular normal matrix, beside a disc whose fits are accepted."""
    X1, X2, phi, dx, dy, layers = _deformed(ny, nx)
    x = np.linspace(0.0, 1.0, nx); y = np.linspace(0.0, 1.0, ny)
    X, Y = np.meshgrid(x, y)
    phi = phi.copy()
    phi[8, 6:9] = -1.0   # three collinear solid cells: det(Aw) = 0 for a fit that sees only them
    solid = (phi < 0).astype(float)
    return (X + 0.01 * Y) * solid, (Y - 0.02 * X) * solid, phi, dx, dy, layers


def _pockets(ny=40, nx=48):
    """Solid everywhere but three fluid pockets: two single cells (4, 3) apart -- the second's
    only source is the first, at the second position of its window, before 79 solid cells:
    the longest tail a record can have, 10 chunks -- and a 2 x 3 block.  8 fits in all, none
    in layers 1 and 2."""
    x = np.linspace(0.0, 1.0, nx); y = np.linspace(0.0, 1.0, ny)
    X, Y = np.meshgrid(x, y)
    phi = -np.ones((ny, nx))
    phi[10, 10] = phi[14, 13] = 1.0
    phi[25:27, 30:33] = 1.0
    solid = (phi < 0).astype(float)
    X1 = X + 0.05 * np.sin(2 * np.pi * Y) * np.cos(np.pi * X)
    X2 = Y + 0.03 * np.sin(2 * np.pi * X)
    return X1 * solid, X2 * solid, phi, 1.0 / (nx - 1), 1.0 / (ny - 1), 3


_CASES = {
    "pockets": lambda oracle: _pockets(),
    "driver33": lambda oracle: _driver33(oracle),
    "disc64": lambda oracle: _deformed(64, 64),
    "disc96x80": lambda oracle: _deformed(96, 80),
    "thin64": lambda oracle: _thin(),
    "disc512": lambda oracle: _deformed(512, 512),
}
_STATE = {}


def _case(oracle, name):
    """Inputs and the oracle's serial result, computed once and never written to."""
    if name not in _STATE:
        X1, X2, phi, dx, dy, layers = _CASES[name](oracle)
        r1, r2 = oracle.extrapolate_reference_map(X1, X2, phi, dx, dy, layers)
        for a in (X1, X2, phi, r1, r2):
            a.setflags(write=False)
        _STATE[name] = (X1, X2, phi, dx, dy, layers, r1, r2)
    return _STATE[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _extrapolate(gpu, case, waves, cols, lgroups):
    """One extrapolation on a context of its own with the options set through the API; the
    chain must have run (path 0) and the call must not have aborted (it raises)."""
    import ctypes
    import torch
    from pyrmt_amd import _lib as L
    from pyrmt_amd import functions as F
    X1, X2, phi, dx, dy, layers = case[:6]
    c = F._Ctx(phi.shape[0], phi.shape[1], torch.cuda.current_device())
    c.set_option("chain_waves", waves)
    c.set_option("chain_cols", cols)
    c.set_option("chain_layer_groups", lgroups)
    assert c.get_option("chain_waves") == waves
    t = [torch.from_numpy(np.array(a, dtype=np.float64)).cuda() for a in (X1, X2, phi)]
    o1, o2 = torch.empty_like(t[0]), torch.empty_like(t[0])
    L.check(L.lib().rmt_extrapolate_reference_map(c.bind(), F._p(t[0]), F._p(t[1]), F._p(t[2]),
                                                  dx, dy, int(layers), F._p(o1), F._p(o2)),
            "extrapolate_reference_map")   # (an abort word is RMT_EDEVICE: raises)
    p = ctypes.c_int(-1)
    L.check(L.lib().rmt_extrap_last_path(c.bind(), ctypes.byref(p)), "rmt_extrap_last_path")
    assert p.value == 0, f"chain path not taken (path {p.value})"
    return o1.cpu().numpy(), o2.cpu().numpy()


def _three_ways(gpu, case, cols, lgroups):
    r1, r2 = case[6:8]
    a1, a2 = _extrapolate(gpu, case, 8, cols, lgroups)
    b1, b2 = _extrapolate(gpu, case, 16, cols, lgroups)
    for name, x, y in (("X1 8 vs 16", a1, b1), ("X2 8 vs 16", a2, b2),
                       ("X1 8 vs oracle", a1, r1), ("X2 8 vs oracle", a2, r2),
                       ("X1 16 vs oracle", b1, r1), ("X2 16 vs oracle", b2, r2)):
        assert np.array_equal(_bits(x), _bits(y)), name


# ------------------------------------------------------------------ the tests --------
def test_option_values(gpu):
    from pyrmt_amd import functions as F
    c = F._Ctx(64, 64, 0)
    assert c.get_option("chain_waves") in (8, 16)
    for w in (8, 16):
        c.set_option("chain_waves", w)
        assert c.get_option("chain_waves") == w
    for bad in (0, 4, 12, 32, -8):
        with pytest.raises(ValueError, match="chain_waves"):
            c.set_option("chain_waves", bad)
        assert c.get_option("chain_waves") == 16


_PARTS_CASES = ["driver33", "disc64", "disc96x80", "pockets"]


@pytest.mark.parametrize("lgroups", [0, 1])
@pytest.mark.parametrize("cols", [1, 2, 3])
@pytest.mark.parametrize("name", _PARTS_CASES)
def test_parts(gpu, oracle, name, cols, lgroups):
    case = _case(oracle, name)
    _three_ways(gpu, case, cols, lgroups)


def test_parts_cover_small_empty_and_cross_part(oracle):
    """What test_parts' grid of options has to contain (CPU): a part with fewer fits than 8
    waves and one with fewer than 16, an empty part, and cross-part sources."""
    small8 = small16 = empty = far = 0
    for name in _PARTS_CASES:
        case = _case(oracle, name)
        for cols in (1, 2, 3):
            for lgroups in (0, 1):
                m = _chain_model(case[2], case[3], case[4], case[5], cols, lgroups)
                n = m["parts"][:m["nparts"]]
                small8 += int(((n > 0) & (n < 8)).sum())
                small16 += int(((n > 0) & (n < 16)).sum())
                empty += int((n == 0).sum())
                far += m["far"]
    print(f"parts with 1..7 fits {small8}, 1..15 fits {small16}, empty {empty}, "
          f"cross-part sources {far}")
    assert small8 > 0 and small16 > 0 and empty > 0 and far > 0


def test_rejected_target(gpu, oracle):
    case = _case(oracle, "thin64")
    m = _chain_model(case[2], case[3], case[4], case[5], 2, 0)
    print(f"thin64: {len(m['fits'])} accepted fits, {m['rejected']} rejected targets")
    assert m["rejected"] > 0 and len(m["fits"]) > 16
    for cols, lgroups in ((2, 0), (1, 1)):
        _three_ways(gpu, case, cols, lgroups)


def test_tails(gpu, oracle):
    """disc96x80 at the default parts: the three tail shapes, found on the CPU."""
    case = _case(oracle, "disc96x80")
    m = _chain_model(case[2], case[3], case[4], case[5], 2, 0)
    last, one, longest = _tails(m)
    print(f"disc96x80: critical term last in {last} fits, single tail chunk in {one}, "
          f"longest tail {longest} chunks")
    # 16 waves keep 3 tail chunks in registers: a longer tail is the part of the fold that
    # moves from LDS into registers at 8 waves
    assert last > 0 and one > 0 and longest > 3
    _three_ways(gpu, case, 2, 0)
    # ... and the longest tail any record can have: 80 terms, the critical one first
    case = _case(oracle, "pockets")
    m = _chain_model(case[2], case[3], case[4], case[5], 1, 1)
    assert _tails(m)[2] == 10 and m["parts"][0] == 8
    _three_ways(gpu, case, 1, 1)


def test_ring_wrap(gpu, oracle):
    """One part of more than CH_R fits: ring slots are reused and a wave more than CH_R / 2
    ahead of the slowest one waits for the watermark."""
    case = _case(oracle, "disc512")
    m = _chain_model(case[2], case[3], case[4], case[5], 1, 1)
    print(f"disc512: fits per part {m['parts'][:m['nparts']]}")
    assert m["nparts"] == 1 and m["parts"][0] > CH_R
    _three_ways(gpu, case, 1, 1)


FIELDS = ("u", "v", "p", "X1", "X2", "phi", "J")


def test_fused_step(gpu):
    import ctypes
    from pyrmt_amd import _lib as L
    from pyrmt_amd.simulation import soft_disc_in_lid_driven
    out = {}
    for w in (8, 16):
        s = soft_disc_in_lid_driven(128, options={"chain_waves": w})
        assert s.ctx.get_option("chain_waves") == w
        s.step(3)
        out[w] = {f: s.get(f) for f in FIELDS}
        out[w].update({"d_" + k: np.asarray(v) for k, v in s.diagnostics().items()})
        # the workspace of the step's last geometry: the chain's records, no fallback flag
        p = ctypes.c_int(-1)
        L.check(L.lib().rmt_extrap_last_path(s.ctx.bind(), ctypes.byref(p)))
        assert p.value == 0, f"chain path not taken at {w} waves (path {p.value})"
    assert sorted(out[8]) == sorted(out[16])
    for k in out[16]:
        assert np.array_equal(_bits(out[8][k]), _bits(out[16][k])), k


def test_slab_step_one_rank(gpu):
    """The slab path at one rank, at N = 256: its DCT-I needs 2 (N - 1) in radices <= 23,
    which 2 * 127 is not."""
    from pyrmt_amd import distributed as D
    out = {}
    for w in (8, 16):
        s = D.soft_disc_in_lid_driven(256, D.LocalComm(1), options={"chain_waves": w})
        s.step(3)
        out[w] = {f: s.gather(f) for f in ("u", "v", "p", "X1", "X2")}
        out[w].update({"d_" + k: np.asarray(v) for k, v in s.diagnostics().items()})
    assert out[16]["d_fitted"][-1] > 0
    for k in out[16]:
        assert np.array_equal(_bits(out[8][k]), _bits(out[16][k])), k
