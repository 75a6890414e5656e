"""The lid-tier wrappers of pyrmt_amd.mac bind a square N x N context and their kernels index
every array by N alone, while the reference accepts Ny != Nx.  A rectangular or mismatched
input has to raise NotImplementedError from the host-side shape check, before any library
call: the library and the context cache are replaced by a tripwire here, so the raise can only
come from that check (and nothing is launched on arrays the kernels would overrun).  No GPU."""
import numpy as np
import pytest

NY, NX = 6, 8


@pytest.fixture
def M(monkeypatch):
    from pyrmt_amd import mac

    def tripwire(*a, **k):
        raise AssertionError("a library call was reached with unchecked shapes")
    monkeypatch.setattr(mac.L, "lib", tripwire)
    monkeypatch.setattr(mac, "ctx_for", tripwire)
    monkeypatch.setattr(mac, "_ctx", tripwire)
    return mac


def _z(*shape):
    return np.zeros(shape)


U, V, P = _z(NY, NX + 1), _z(NY + 1, NX), _z(NY, NX)     # the reference's layout at Ny != Nx
SQ_U, SQ_V, SQ_P = _z(NY, NY + 1), _z(NY + 1, NY), _z(NY, NY)
PRED = (0.01, 0.1, 0.1, 1e-3, 1.0)                       # nu, dx, dy, dt, U_lid

# case -> (the function the message names, the call)
CASES = {
    "divergence": ("divergence", lambda m: m.divergence(U, V, 0.1, 0.1)),
    "divergence_mismatch": ("divergence",
                            lambda m: m.divergence(SQ_U, _z(NY + 1, NY + 1), 0.1, 0.1)),
    "gradient_p_u": ("gradient_p_u", lambda m: m.gradient_p_u(P, 0.1)),
    "gradient_p_v": ("gradient_p_v", lambda m: m.gradient_p_v(P, 0.1)),
    "project": ("project", lambda m: m.project(U, V, 0.1, 0.1, 1e-3, 1.0, P + 1.0)),
    "project_eig": ("project", lambda m: m.project(SQ_U, SQ_V, 0.1, 0.1, 1e-3, 1.0, P + 1.0)),
    "solve_eig": ("solve_poisson_neumann", lambda m: m.solve_poisson_neumann(P, SQ_P + 1.0)),
    "solve_1d": ("solve_poisson_neumann", lambda m: m.solve_poisson_neumann(_z(NX), _z(NX))),
    "predictor": ("momentum_predictor", lambda m: m.momentum_predictor(U, V, *PRED)),
    "predictor_force": ("momentum_predictor",
                        lambda m: m.momentum_predictor(SQ_U, SQ_V, *PRED, fu=SQ_U, fv=V)),
    "lid_imex": ("momentum_predictor_lid_imex",
                 lambda m: m.momentum_predictor_lid_imex(U, V, *PRED)),
    "lid_imex_force": ("momentum_predictor_lid_imex",
                       lambda m: m.momentum_predictor_lid_imex(SQ_U, SQ_V, *PRED, fu=U, fv=SQ_V)),
    "lid_semilag": ("momentum_predictor_lid_semilag",
                    lambda m: m.momentum_predictor_lid_semilag(U, V, *PRED)),
    "lap_u": ("_lap_u_lid_hom", lambda m: m._lap_u_lid_hom(U, 0.1, 0.1)),
    "lap_v": ("_lap_v_lid_hom", lambda m: m._lap_v_lid_hom(V, 0.1, 0.1)),
    "contact_stress": ("contact_stress",
                       lambda m: m.contact_stress(P, P, 2.0, 0.6, 0.3, 0.1, 0.1)),
    "contact_stress_mismatch": ("contact_stress",
                                lambda m: m.contact_stress(SQ_P, P, 2.0, 0.6, 0.3, 0.1, 0.1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_wrapper_refuses_before_any_library_call(M, name):
    what, call = CASES[name]
    with pytest.raises(NotImplementedError) as e:
        call(M)
    msg = str(e.value)       # "<function>: ... <the shapes it was given>"
    assert msg.startswith(what + ":"), msg
    assert any(str(np.shape(a)) in msg for a in (P, U, V, _z(NX), _z(NY + 1, NY + 1))), msg


def test_square_inputs_pass_the_check(M):
    """The check lets the square layout through and returns its N."""
    assert M._lid_n("t", SQ_U, SQ_V, SQ_U, SQ_V, eig=SQ_P) == NY
    assert M._lid_n("t", v=SQ_V) == NY
    assert M._lid_n("t", phi_a=SQ_P, phi_b=SQ_P) == NY
