"""Fitting the constants of a hand-written SDE to data, THROUGH `sdeint`: the stochastic Lorenz system of the reference's
examples/latent_sde_lorenz.py:56-86 as an `nn.Module` with its constants as parameters, written the way that example writes it
(`split`, arithmetic among the columns, `cat`). Its channels read each other, so it is no elementwise program: the column
interpreter (recognise_rows.py) turns it into a generated kernel in which one lane owns a whole row, and with autograd recording
that kernel carries forward-mode tangents -- d/dy0 and one per parameter -- in registers beside the state. One launch forward, a
few reductions backward, no step stored. (The first solve compiles the kernel, a few seconds, and runs both routes to compare.)

Here: paths sampled from the module with the true drift constants (10, 28, 8/3), and a second module that starts elsewhere and
recovers them from those paths, driven by the same Brownian motion.

    python examples/fit_lorenz_parameters.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout

import torch
from torch import nn

import torchsde_amd as torchsde  # noqa: E402
from torchsde_amd import recognise  # noqa: E402


class Lorenz(nn.Module):
    noise_type, sde_type = "diagonal", "ito"

    def __init__(self, a=(10.0, 28.0, 8.0 / 3.0), b=(0.1, 0.28, 0.3)):
        super().__init__()
        self.a = nn.Parameter(torch.tensor(a))
        self.b = nn.Parameter(torch.tensor(b))

    def f(self, t, y):
        x1, x2, x3 = torch.split(y, (1, 1, 1), dim=1)
        a1, a2, a3 = self.a
        return torch.cat([a1 * (x2 - x1), a2 * x1 - x2 - x1 * x3, x1 * x2 - a3 * x3], dim=1)

    def g(self, t, y):
        return y * self.b


if __name__ == "__main__":
    device = "cuda"
    batch, dt, t1 = 4096, 2.0 ** -8, 0.25
    torch.manual_seed(0)
    target = Lorenz().to(device)
    model = Lorenz(a=(8.0, 24.0, 2.0)).to(device)
    y0 = torch.randn(batch, 3, device=device)
    ts = torch.linspace(0.0, t1, 5, device=device)

    def path(sde):
        # (the same entropy: the same Brownian motion for the data and for every fit)
        bm = torchsde.BrownianInterval(0.0, t1, size=(batch, 3), device=device, entropy=11)
        return torchsde.sdeint(sde, y0, ts, bm=bm, method="euler", dt=dt)

    with torch.no_grad():
        data = path(target)
    optimiser = torch.optim.Adam([model.a], lr=0.2)
    for it in range(301):
        optimiser.zero_grad()
        ys = path(model)
        loss = (ys - data).square().mean()
        loss.backward()
        optimiser.step()
        if it % 50 == 0:
            route = type(ys.grad_fn).__name__
            print(f"step {it:3d}  loss {loss.item():.3e}  a = {[round(v, 3) for v in model.a.tolist()]}  ({route})")
    print("true drift constants:", [round(v, 3) for v in target.a.tolist()])
    for line in recognise.describe(model):
        print(line)
