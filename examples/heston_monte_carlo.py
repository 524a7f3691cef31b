"""Monte Carlo under the Heston model: a hand-written module with a diffusion MATRIX -- two correlated Brownian channels,
noise type "general" -- goes through `sdeint` unchanged, and the whole solve is one launch of a kernel generated from the
module's own `f` and `g` (one lane per path; the matrix's structural zero costs nothing).

    ds = mu s dt + s sqrt(v) dW1
    dv = kappa (theta - v) dt + xi sqrt(v) (rho dW1 + sqrt(1 - rho^2) dW2)

The first solve of a module runs both routes, compares them and returns the stepwise result; `recognise.describe` says what was
decided. (Euler: the scheme for Ito general noise. The generated unit compiles in the background and solves stay stepwise
until it is there; this script compiles it in its own thread.)

    python examples/heston_monte_carlo.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout

import math
import time

import torch
from torch import nn

import torchsde_amd as torchsde  # noqa: E402


class Heston(nn.Module):
    noise_type, sde_type = "general", "ito"

    def __init__(self, mu=0.03, kappa=2.0, theta=0.09, xi=0.3, rho=-0.7):
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
        root = torch.sqrt(torch.relu(v))                       # (full truncation: the variance may touch zero)
        first = torch.stack([s * root, torch.zeros_like(s)], dim=1)
        second = torch.stack([self.xi * self.rho * root, self.xi * torch.sqrt(1 - self.rho ** 2) * root], dim=1)
        return torch.stack([first, second], dim=1)              # (paths, 2, 2)


if __name__ == "__main__":
    from torchsde_amd import specialise
    specialise.MODE = "sync"                                    # compile the generated unit in this thread
    device = "cuda"
    paths, steps, maturity, strike = 1 << 16, 1000, 1.0, 1.0
    sde = Heston().to(device)
    y0 = torch.tensor([1.0, 0.09], device=device).expand(paths, 2).contiguous()
    ts = torch.tensor([0.0, maturity], device=device)
    for solve in range(3):
        bm = torchsde.BrownianInterval(0.0, maturity, size=(paths, 2), device=device, dtype=torch.float32, entropy=7 + solve)
        torch.cuda.synchronize()
        t = time.perf_counter()
        with torch.no_grad():
            ys = torchsde.sdeint(sde, y0, ts, bm=bm, method="euler", dt=maturity / steps)
        torch.cuda.synchronize()
        price = torch.relu(ys[-1, :, 0] - strike).mean().item() * math.exp(-sde.mu.item() * maturity)
        print(f"solve {solve}: {paths} paths x {steps} Euler steps in {(time.perf_counter() - t) * 1e3:8.1f} ms, "
              f"call price {price:.4f}" + ("   (both routes, compared)" if solve == 0 else ""))
    for line in torchsde.recognise.describe(sde):
        print(line)
