"""Golden-vector generator for the free-slip MAC box (pyRMT/mac.py:179-193, 656-689 and the
drivers benchmarks/mac_disc_in_tg_convergence.py, benchmarks/mac_two_disc_contact.py): runs the
pyRMT reference in pure-Python mode (imported exactly as gen_golden.py does) and writes

    tests/golden/mac_freeslip_ops.npz      the two operators at N = 4, 5, 33
    tests/golden/mac_freeslip_ops64.npz    ... at N = 64
    tests/golden/mac_freeslip_drop.npz     one composed static-drop step at N = 40
    tests/golden/mac_freeslip_tg.npz       disc in vortex: run_one(N, (n + 0.5) dt)
    tests/golden/mac_freeslip_contact.npz  two discs: run(N=32, t_end=0.2, V0=0.5), eta 2 and 0

The drivers' loop bodies are not restated: their own run_one / run are called, and state is
captured by wrapping the names the driver modules imported (project: u, v, p of each step;
extrapolate_reference_map: X1, X2; solid_cauchy_stress: the J range; contact_stress: the count
of non-zero cells).  Every case is run a second time with the first predictor call's u, v
moved by one ulp (nextafter): the difference is the reference's own noise floor, stored as
noise_* and required to be at most a tenth of the bar the GPU tests hold to (the J range: a
fifth, see gen_tg).  Every file stays
under 600 KB.

This script is TEST INFRASTRUCTURE, run only where the reference is present; the committed
.npz files are data.

Usage:  python -B tests/golden/gen_mac_freeslip.py
"""
import contextlib
import io
import os
import sys
import tempfile
import time

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import F, M, OUT, save  # noqa: E402
import numpy as np  # noqa: E402
import benchmarks.mac_disc_in_tg_convergence as TG  # noqa: E402
import benchmarks.mac_two_disc_contact as TD  # noqa: E402

OPS_N = (4, 5, 33, 64)
NU, DT, RHO, GAMMA = 0.01, 1e-3, 1.3, 0.07
TG_CASES = ((32, 24), (33, 24), (64, 40))       # (N, n): t_end = (n + 0.5) dt
# the bars of tests/test_gpu_mac_freeslip.py; the noise floor must stay a tenth below each
BAR_FIELD, BAR_KE, BAR_ES, BAR_HIST, BAR_J = 1e-9, 1e-9, 1e-7, 1e-10, 1e-9


def gen_ops(N, seed):
    rng = np.random.default_rng(seed)
    dx, dy = M.mac_grid(N, N)
    # (the wall-normal faces are not zeroed: the outputs' zeroing is under test)
    u, fu = rng.standard_normal((2, N, N + 1))
    v, fv = rng.standard_normal((2, N + 1, N))
    kappa, H = rng.standard_normal((2, N, N))
    us, vs = M.momentum_predictor_freeslip(u, v, NU, dx, dy, DT, fu=fu, fv=fv, rho=RHO)
    us0, vs0 = M.momentum_predictor_freeslip(u, v, NU, dx, dy, DT)
    gu, gv = M.interfacial_force_faces(kappa, H, GAMMA, dx, dy)
    return dict(u=u, v=v, fu=fu, fv=fv, kappa=kappa, H=H, us=us, vs=vs, us0=us0, vs0=vs0,
                gu=gu, gv=gv)


def gen_drop(N=40, R=0.25, gamma=0.05, nu=0.01, rho=1.0, dt=1e-3):
    """One static-drop step composed of the reference's operators, every intermediate kept."""
    dx, dy = M.mac_grid(N, N)
    xc = (np.arange(N) + 0.5) * dx
    Xc, Yc = np.meshgrid(xc, xc)
    phi = np.sqrt((Xc - 0.5) ** 2 + (Yc - 0.5) ** 2) - R
    kappa = F.compute_curvature(phi, dx, dy)
    H = F.smoothed_heaviside(phi, 2.0 * dx)
    fu, fv = M.interfacial_force_faces(kappa, H, gamma, dx, dy)
    u0 = np.zeros((N, N + 1)); v0 = np.zeros((N + 1, N))
    us, vs = M.momentum_predictor_freeslip(u0, v0, nu, dx, dy, dt, fu=fu, fv=fv, rho=rho)
    u, v, p = M.project(us, vs, dx, dy, dt, rho, M.poisson_eigs_neumann(N, N, dx, dy))
    assert np.abs(us).max() > 0 and np.abs(p).max() > 0
    save("mac_freeslip_drop", N=N, R=R, gamma=gamma, nu=nu, rho=rho, dt=dt, phi=phi, kappa=kappa,
         H=H, fu=fu, fv=fv, us=us, vs=vs, u=u, v=v, p=p)


@contextlib.contextmanager
def wrapped(mod, perturb, st):
    """The driver module's imported names wrapped to record what passes through them."""
    names = ("momentum_predictor_freeslip", "project", "extrapolate_reference_map",
             "solid_cauchy_stress") + (("contact_stress",) if hasattr(mod, "contact_stress") else ())
    orig = {n: getattr(mod, n) for n in names}
    st.update(calls=0, J=[], stepJ=[1.0, 1.0], cells=[], maps=[])

    def pred(u, v, *a, **k):
        if perturb and st["calls"] == 0:
            u = np.nextafter(u, np.inf); v = np.nextafter(v, -np.inf)
        st["calls"] += 1
        st["dt_last"] = a[3]
        st["J"].append(tuple(st["stepJ"])); st["stepJ"] = [1.0, 1.0]
        st["end_maps"] = st["maps"]; st["maps"] = []
        return orig["momentum_predictor_freeslip"](u, v, *a, **k)

    def proj(*a, **k):
        st["uvp"] = orig["project"](*a, **k)
        return st["uvp"]

    def extrap(*a, **k):
        r = orig["extrapolate_reference_map"](*a, **k)
        st["maps"].append(r)
        return r

    def stress(*a, **k):
        r = orig["solid_cauchy_stress"](*a, **k)
        st["stepJ"] = [min(st["stepJ"][0], r[3].min()), max(st["stepJ"][1], r[3].max())]
        return r

    def contact(*a, **k):
        r = orig["contact_stress"](*a, **k)
        st["cells"].append(int(np.count_nonzero(r[0])))
        return r

    new = dict(momentum_predictor_freeslip=pred, project=proj, extrapolate_reference_map=extrap,
               solid_cauchy_stress=stress, contact_stress=contact)
    for n in names:
        setattr(mod, n, new[n])
    try:
        yield
    finally:
        for n in names:
            setattr(mod, n, orig[n])


def tg_dt(N):
    dx = 1.0 / N
    return min(0.25 * dx / (0.3 * np.pi), 0.2 * dx * dx / 0.01, 0.25 * dx / (np.sqrt(0.1) + 1e-9))


def run_tg(N, n, perturb):
    st = {}
    with wrapped(TG, perturb, st):
        r = TG.run_one(N, (n + 0.5) * tg_dt(N))
    assert st["calls"] == n + 1, st["calls"]
    (X1, X2), = st["end_maps"]
    return r, st, X1, X2


def gen_tg(out):
    for N, n in TG_CASES:
        a, sa, X1, X2 = run_tg(N, n, False)
        b, sb, Y1, Y2 = run_tg(N, n, True)
        u, v, p = sa["uvp"]
        noise_f = max(np.abs(x - y).max() for x, y in zip((u, v, X1, X2), sb["uvp"][:2] + (Y1, Y2)))
        noise_p = np.abs(p - sb["uvp"][2]).max()
        noise_ke = abs(a["KE"] - b["KE"]) / a["KE"]
        noise_es = abs(a["Estrain"] - b["Estrain"]) / a["Estrain"]
        J = np.array(sa["J"]); Jb = np.array(sb["J"])
        noise_j = np.abs(J / Jb - 1).max()
        print(f"  disc in vortex N={N}: {n + 1} steps, noise fields {noise_f:.2g} p {noise_p:.2g} "
              f"KE {noise_ke:.2g} Estrain {noise_es:.2g} J {noise_j:.2g}; J in "
              f"[{J[:, 0].min():.4f}, {J[:, 1].max():.4f}], divmax {a['divmax']:.2g}")
        assert noise_f <= 0.1 * BAR_FIELD and noise_p <= 0.1 * BAR_FIELD
        assert noise_ke <= 0.1 * BAR_KE and noise_es <= 0.1 * BAR_ES
        # J is a difference quotient of the map (its noise is the map's times 1 / dx): a fifth
        # of its 1e-9 bar (measured: 0.11 of it at N = 64, below 0.012 at N = 32, 33)
        assert noise_j <= 0.2 * BAR_J
        assert np.array_equal(a["p"], p) and a["divmax"] < 1e-9 and a["Estrain"] > 0
        phi = np.sqrt((X1 - 0.5) ** 2 + (X2 - 0.7) ** 2) - 0.15
        d = dict(n=n, dt=tg_dt(N), dt_last=sa["dt_last"], u=u, v=v, p=p, X1=X1, X2=X2, phi=phi,
                 KE=a["KE"], Estrain=a["Estrain"], divmax=a["divmax"], J=J, noise_fields=noise_f,
                 noise_p=noise_p, noise_KE=noise_ke, noise_Estrain=noise_es, noise_J=noise_j)
        out.update({f"n{N}_{k}": val for k, val in d.items()})
    out["cases"] = np.array(TG_CASES)


def run_td(eta, perturb, tmp):
    st = {}
    with wrapped(TD, perturb, st), contextlib.redirect_stdout(io.StringIO()):
        h = TD.run(N=32, t_end=0.2, V0=0.5, eta=eta, out_root=tmp)
    return h, st


def gen_contact():
    dx = 1.0 / 32
    dt = min(0.25 * dx / 0.5, 0.2 * dx * dx / 0.02, 0.25 * dx / (np.sqrt(0.2) + 1e-9))
    with tempfile.TemporaryDirectory() as tmp:
        h2, s2 = run_td(2.0, False, tmp)
        h2n, s2n = run_td(2.0, True, tmp)
        h0, s0 = run_td(0.0, False, tmp)
        h0n, s0n = run_td(0.0, True, tmp)
    out = dict(N=32, t_end=0.2, V0=0.5, dt=dt)
    for tag, h, s, hn, sn in (("eta2", h2, s2, h2n, s2n), ("eta0", h0, s0, h0n, s0n)):
        nf = max(np.abs(x - y).max() for x, y in zip(s["uvp"][:2], sn["uvp"][:2]))
        nh = np.abs(h / hn - 1).max()
        print(f"  two discs {tag}: {len(h)} steps, gap {h[0, 3]:.4f} -> {h[-1, 3]:.4f}, noise u, v "
              f"{nf:.2g}, history {nh:.2g}")
        assert nf <= 0.1 * BAR_FIELD and nh <= 0.1 * BAR_HIST
        out.update({f"{tag}_hist": h, f"{tag}_u": s["uvp"][0], f"{tag}_v": s["uvp"][1],
                    f"{tag}_noise_fields": nf, f"{tag}_noise_hist": nh})
    # the contact term is active on every step, and eta changes the flow
    cells = np.array(s2["cells"])
    effect = np.abs(s2["uvp"][0] - s0["uvp"][0]).max()
    print(f"  contact cells per step {cells.min()}..{cells.max()}, eta effect on u {effect:.2g}")
    assert len(cells) == len(h2) and cells.min() > 0 and not s0["cells"]
    assert effect > 1e-2
    out.update(cells=cells, eta_effect=effect)
    save("mac_freeslip_contact", **out)


if __name__ == "__main__":
    t0 = time.time()
    small = {}
    for k, N in enumerate(OPS_N):
        d = gen_ops(N, 9100 + k)
        if N == 64:
            save("mac_freeslip_ops64", N=N, nu=NU, dt=DT, rho=RHO, gamma=GAMMA, **d)
        else:
            small.update({f"n{N}_{key}": val for key, val in d.items()})
    save("mac_freeslip_ops", Ns=np.array(OPS_N[:3]), nu=NU, dt=DT, rho=RHO, gamma=GAMMA, **small)
    gen_drop()
    tg = {}
    gen_tg(tg)
    save("mac_freeslip_tg", **tg)
    gen_contact()
    for f in ("ops", "ops64", "drop", "tg", "contact"):
        size = os.path.getsize(os.path.join(OUT, f"mac_freeslip_{f}.npz"))
        assert size <= 600 * 1024, (f, size)
    print(f"done in {time.time() - t0:.0f}s")
