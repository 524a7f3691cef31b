"""Small row-coupled systems with a diffusion MATRIX -- general, scalar and additive noise -- as users write them: the modules of
tests/test_recognise_rows_general.py and tests/test_gpu_rows_general.py, and the dense worst case whose generated unit
tools/rows_general_resource_usage.py compiles (torchsde_amd/recognise_rows.py `recognise_rows(..., m=m)`,
specialise.source_rows_general)."""
import math

import torch
from torch import nn


class Heston(nn.Module):
    """ds = mu s dt + s sqrt(v) dW1,  dv = kappa (theta - v) dt + xi sqrt(v) (rho dW1 + sqrt(1 - rho^2) dW2): two correlated
    Brownian channels, one structural zero in the diffusion matrix."""
    noise_type, sde_type = "general", "ito"
    d, m = 2, 2
    y0 = (1.0, 0.5)

    def __init__(self, mu=0.05, kappa=2.0, theta=0.5, xi=0.3, rho=-0.7):
        super().__init__()
        self.mu = nn.Parameter(torch.tensor(float(mu)))
        self.kappa = nn.Parameter(torch.tensor(float(kappa)))
        self.theta = nn.Parameter(torch.tensor(float(theta)))
        self.xi = nn.Parameter(torch.tensor(float(xi)))
        self.rho = nn.Parameter(torch.tensor(float(rho)))

    def f(self, t, y):
        s, v = y[:, 0], y[:, 1]
        return torch.stack([self.mu * s, self.kappa * (self.theta - v)], dim=1)

    def g(self, t, y):
        s, v = y[:, 0], y[:, 1]
        root = torch.sqrt(v)
        first = torch.stack([s * root, torch.zeros_like(s)], dim=1)
        second = torch.stack([self.xi * self.rho * root, self.xi * torch.sqrt(1 - self.rho ** 2) * root], dim=1)
        return torch.stack([first, second], dim=1)


class Dense(nn.Module):
    """f_i = -y_i + a y_(i+1)%d cos(t),  g_ik = S_ik tanh(y_(i+k)%d)  with an asymmetric S: a transposed layout cannot pass.
    g is assembled by `reshape` of a `cat` of columns."""
    noise_type = "general"

    def __init__(self, d, m, sde_type):
        super().__init__()
        self.d, self.m, self.sde_type = d, m, sde_type
        self.y0 = tuple(0.3 + 0.1 * c for c in range(d))
        self.a = nn.Parameter(torch.tensor(0.5))
        i, k = torch.meshgrid(torch.arange(d), torch.arange(m), indexing="ij")
        self.S = nn.Parameter(0.1 + 0.05 * i + 0.02 * k * k - 0.03 * i * k)

    def f(self, t, y):
        d = self.d
        return torch.cat([-y[:, i:i + 1] + self.a * y[:, (i + 1) % d:(i + 1) % d + 1] * torch.cos(t) for i in range(d)], dim=1)

    def g(self, t, y):
        d, m = self.d, self.m
        cols = [self.S[i, k] * torch.tanh(y[:, (i + k) % d:(i + k) % d + 1]) for i in range(d) for k in range(m)]
        return torch.cat(cols, dim=1).reshape(y.shape[0], d, m)


class ScalarVanDerPol(nn.Module):
    """x' = v, v' = mu (1 - x^2) v - x, both driven by ONE Brownian channel."""
    noise_type = "scalar"
    d, m = 2, 1
    y0 = (0.5, -0.2)

    def __init__(self, sde_type="ito"):
        super().__init__()
        self.sde_type = sde_type
        self.mu = nn.Parameter(torch.tensor(1.5))
        self.sigma = nn.Parameter(torch.tensor([0.2, 0.3]))

    def f(self, t, y):
        x, v = y[:, 0], y[:, 1]
        return torch.stack([v, self.mu * (1 - x ** 2) * v - x], dim=1)

    def g(self, t, y):
        x, v = y[:, 0], y[:, 1]
        return torch.stack([self.sigma[0] * torch.tanh(v), self.sigma[1] * torch.sigmoid(x)], dim=1).unsqueeze(-1)


class Langevin(nn.Module):
    """Two underdamped oscillators (q1, q2, p1, p2): additive noise that enters the momentum rows only -- the upper half of
    the diffusion matrix is structurally zero. `timed`: the noise decays as exp(-t)."""
    noise_type = "additive"
    d, m = 4, 2
    y0 = (0.4, -0.3, 0.1, 0.2)

    def __init__(self, sde_type="ito", timed=True):
        super().__init__()
        self.sde_type, self.timed = sde_type, timed
        self.gamma = nn.Parameter(torch.tensor(0.7))
        self.k = nn.Parameter(torch.tensor([1.3, 0.8]))
        self.sigma = nn.Parameter(torch.tensor([[0.3, 0.1], [-0.2, 0.25]]))

    def f(self, t, y):
        q, p = y[:, :2], y[:, 2:]
        return torch.cat([p, -self.k * q - self.gamma * p - 0.1 * q ** 3], dim=1)

    def g(self, t, y):
        B = y.shape[0]
        sigma = self.sigma * torch.exp(-t) if self.timed else self.sigma
        return torch.cat([torch.zeros(B, 2, 2, dtype=y.dtype, device=y.device), sigma.expand(B, 2, 2)], dim=1)


class DenseWorst(nn.Module):
    """The worst case of a size: every drift channel and every entry of the diffusion matrix reads every state channel, a
    constant of its own and t, through a transcendental function (tools/rows_general_resource_usage.py)."""
    noise_type, sde_type = "general", "stratonovich"

    def __init__(self, d, m):
        super().__init__()
        self.d, self.m = d, m
        self.A = nn.Parameter(torch.linspace(-0.5, 0.5, d * d).reshape(d, d))
        self.S = nn.Parameter(torch.linspace(0.1, 0.4, d * m).reshape(d, m))

    def f(self, t, y):
        d = self.d
        bounded = [torch.tanh(c) for c in y.unbind(dim=1)]
        wave = torch.sin(t)
        return torch.stack([sum((self.A[i, j] * bounded[j] for j in range(1, d)), self.A[i, 0] * bounded[0]) + wave
                            for i in range(d)], dim=1)

    def g(self, t, y):
        d, m = self.d, self.m
        cols = list(y.unbind(dim=1))
        total = sum(cols[1:], cols[0])
        wave = torch.cos(t)
        rows = [torch.stack([self.S[i, k] * torch.tanh(total * math.cos(i + 2 * k) + cols[(i + k) % d]) * wave
                             for k in range(m)], dim=1) for i in range(d)]
        return torch.stack(rows, dim=1)


def modules():
    """name -> factory(sde_type) of every test module, with `.d`, `.m`, `.y0`."""
    out = {"heston": lambda sde_type: Heston(), "scalar_vdp": ScalarVanDerPol,
           "langevin": lambda sde_type: Langevin(sde_type), "langevin_untimed": lambda sde_type: Langevin(sde_type, timed=False)}
    for d, m in ((3, 5), (2, 4), (5, 1), (8, 8)):
        out[f"dense_{d}x{m}"] = (lambda d, m: lambda sde_type: Dense(d, m, sde_type))(d, m)
    return out


SCHEMES = {"ito": ("euler",), "stratonovich": ("midpoint", "heun", "euler_heun")}
