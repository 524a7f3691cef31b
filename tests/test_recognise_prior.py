"""The prior drift of a ``logqp=True`` solve as the KL perceptron kernels take it (torchsde_amd/recognise.py:
``recognise_prior``, ``prior_coefficient_graph``; the route is torchsde_amd/mlp_adjoint.plan_logqp): a per-channel affine
function of y that does not read t is accepted with the right coefficients, everything else is refused with a reason, and the
probe-built coefficient tensors pass a gradient on to whatever parameters the user's code derives them from."""
import pytest
import torch

from torchsde_amd import recognise

D = 6


class _Prior(torch.nn.Module):
    def __init__(self, kind, theta_elements=D):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.kind = kind
        self.theta = torch.nn.Parameter(0.5 + torch.rand(theta_elements, generator=gen))
        self.mu = torch.nn.Parameter(torch.randn(D, generator=gen))
        self.lin = torch.nn.Linear(D, D)

    def h(self, t, y):
        if self.kind == "ou":
            return -self.theta * y
        if self.kind == "mean_reverting":
            return self.theta * (self.mu - y)
        if self.kind == "numbers":
            return -0.5 * y + 0.05
        if self.kind == "minus_y":
            return -y
        if self.kind == "tanh_cos":
            return 0.5 * torch.tanh(y) - 0.1 * torch.cos(t)
        if self.kind == "tanh":
            return 0.5 * torch.tanh(y)
        if self.kind == "times_t":
            return -y * t
        if self.kind == "network":
            return self.lin(y)
        if self.kind == "detached":
            return -self.theta * y.detach()
        raise AssertionError(self.kind)


def _coefficients(module, differentiable=True, rows=None):
    y0 = torch.randn(9, D, generator=torch.Generator().manual_seed(1))
    hr, hs = recognise.recognise_prior(module.h, torch.tensor(0.25), y0, differentiable=differentiable, rows=rows)
    return (recognise.prior_vector(hr, D, torch.float32, y0.device), recognise.prior_vector(hs, D, torch.float32, y0.device))


@pytest.mark.parametrize("differentiable", (False, True))
def test_accepted_forms_have_the_right_coefficients(differentiable):
    m = _Prior("ou")
    hr, hs = _coefficients(m, differentiable)
    assert torch.equal(hr, -m.theta.detach()) and torch.equal(hs, torch.zeros(D))
    for elements in (D, 1):
        m = _Prior("mean_reverting", theta_elements=elements)
        hr, hs = _coefficients(m, differentiable)
        assert hr.shape == hs.shape == (D,)
        assert torch.equal(hr, (-m.theta.detach()).expand(D))
        assert torch.equal(hs, (m.theta * m.mu).detach())
    hr, hs = _coefficients(_Prior("numbers"), differentiable)
    assert torch.equal(hr, torch.full((D,), -0.5)) and torch.equal(hs, torch.full((D,), 0.05))
    hr, hs = _coefficients(_Prior("minus_y"), differentiable)
    assert torch.equal(hr, torch.full((D,), -1.0)) and torch.equal(hs, torch.zeros(D))


def test_coefficients_reproduce_the_prior_on_random_rows():
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(17, D, generator=gen)
    for kind, elements in (("ou", D), ("mean_reverting", D), ("mean_reverting", 1), ("numbers", D), ("minus_y", D)):
        m = _Prior(kind, theta_elements=elements)
        hr, hs = _coefficients(m, rows=5)
        want = m.h(torch.tensor(0.25), y).detach()
        assert torch.allclose(hr * y + hs, want, rtol=1e-6, atol=1e-6), kind


@pytest.mark.parametrize("kind, differentiable, fragment", (
    ("tanh_cos", True, ""),
    ("tanh", True, "tanh"),
    ("times_t", True, "depends on t"),
    ("network", True, "not a per-channel function"),
    ("detached", True, "stop-gradient"),
))
def test_refused_with_a_reason(kind, differentiable, fragment):
    with pytest.raises(recognise.NotElementwise) as e:
        _coefficients(_Prior(kind), differentiable)
    assert str(e.value) and fragment in str(e.value)


def test_a_detached_state_is_no_stop_gradient_when_no_gradient_is_asked():
    m = _Prior("detached")
    hr, _ = _coefficients(m, differentiable=False)
    assert torch.equal(hr, -m.theta.detach())


@pytest.mark.parametrize("kind, elements", (("ou", D), ("mean_reverting", D), ("mean_reverting", 1)))
def test_probe_built_coefficients_backpropagate_to_the_priors_parameters(kind, elements):
    """dL/dhr = sum_rows r y and dL/dhs = sum_rows r for L = <h(t, y), r>: handed to the probe-built tensors, they must reach
    theta and mu as autograd through h itself does."""
    m = _Prior(kind, theta_elements=elements).double()
    gen = torch.Generator().manual_seed(7)
    y = torch.randn(23, D, generator=gen, dtype=torch.float64)
    r = torch.randn(23, D, generator=gen, dtype=torch.float64)
    t = torch.tensor(0.25, dtype=torch.float64)
    params = [m.theta, m.mu]
    want = torch.autograd.grad((m.h(t, y) * r).sum(), params, allow_unused=True)
    hr_t, hs_t = recognise.prior_coefficient_graph(m.h, t, D, torch.float64, y.device)
    assert hr_t.shape == hs_t.shape == (D,)
    have = torch.autograd.grad([hr_t, hs_t], params, grad_outputs=[(r * y).sum(0), r.sum(0)], allow_unused=True)
    for w, h, p in zip(want, have, params):
        w = torch.zeros_like(p) if w is None else w
        h = torch.zeros_like(p) if h is None else h
        assert torch.allclose(h, w, rtol=1e-12, atol=1e-12)


def test_constant_prior_has_no_graph():
    hr_t, hs_t = recognise.prior_coefficient_graph(_Prior("numbers").h, torch.tensor(0.0), D, torch.float32, "cpu")
    assert not hr_t.requires_grad and not hs_t.requires_grad
    assert torch.allclose(hr_t, torch.full((D,), -0.5)) and torch.allclose(hs_t, torch.full((D,), 0.05))
