"""The trust ledger of the recognised routes: which user modules have earned a one-launch kernel, and which stay stepwise.

A recognised route runs a user's unchanged module on a kernel (solvers._integrate_recognised and the routes beside it,
neural_rheun_route.plan). Before a user gets kernel arithmetic the route opens this per-object book (`open_book`), looks up
earlier refusals, interprets the code, looks up the verdict of the form's key -- and on a first solve interprets the code again
on a 5-row probe, checks that the calls left Python-side state and the random generators alone, runs both routes and files
the verdict. The book lives on the user's SDE object, ``base.__dict__["_tsde_recognised"]``:

- "refused": {(Python-side state, wrapper chain, who): reason}, at most 16 entries
- "trusted": {(structure, chain, solver name, sde_type, d, dtype, batch, *tags): True | reason}, at most 32 entries
- "program", "uses_t": (chain, solver name) of code known to end as an expression program / to use t (solvers._interpret);
  "not_rows": of code the differentiable column interpretation does not hold (solvers._integrate_rows_with_grad);
  "rows_general": of code known to end as a row-coupled system with a diffusion matrix (solvers._interpret);
  "autograd": {(chain, solver name): why solves stay stepwise while autograd records}
- "counter_rate": {key: {call counter: advance per step}}, "solves": {key: solves since the last check}, pruned with "trusted"
"""
import torch

from . import graph

ATTR = "_tsde_recognised"

_UNTAKEN = object()


def may_be_interpreted(base):
    """The interpretation CALLS the user's f and g on a two-row probe. Modules for which one extra call is not
    harmless are left alone: compiled modules (a dispatch mode under torch.compile recompiles or fails), and modules
    with normalisation layers in training mode (a call would feed the probe into their running statistics)."""
    if type(base).__name__ == "OptimizedModule":
        return False
    if isinstance(base, torch.nn.Module):
        for m in base.modules():
            if m.training and isinstance(m, torch.nn.modules.batchnorm._NormBase) \
                    and getattr(m, "track_running_stats", False):
                return False
    return True


def rng_states(device):
    """Host-side snapshots of the default CPU and device generators (seed + offset; no device synchronisation)."""
    return torch.get_rng_state(), torch.cuda.get_rng_state(device)


def open_book(solver, keep_counters=False, who=None, create=True):
    """The `Ledger` of the SDE object `solver` integrates, or None when the route stays stepwise: a module that an extra call
    could harm, pure call counters on a route that cannot keep them at the stepwise loop's value (`keep_counters=False`), an
    object that cannot carry the book. `who` names the route in refusal keys (default: the solver's class name);
    `create=False` opens a book that may not exist yet."""
    chain, base = graph._wrapper_chain(solver.sde)
    if not may_be_interpreted(base):
        return None
    # Pure call counters (`self._nfe += 1` in the reference's Ex* test problems): not state of the dynamics (graph.
    # call_counters decides that on the bytecode), so they neither refuse the form nor lose their meaning -- the verifying
    # solve learns by how much the stepwise loop advances them per step, and a kernel solve leaves them at that value.
    # `options={"assume_pure": True}` (or the attribute `tsde_assume_pure = True` on the SDE object): the USER vouches that
    # whatever Python-side state their f and g touch (counters, logs, caches) does not reach the dynamics -- the documented
    # switch for modules the checks below would keep stepwise. Nothing is fingerprinted then, counters run once per solve
    # instead of once per step; the both-routes comparison of the first solve (and TSDE_VERIFY_EVERY) still applies.
    assume_pure = bool(solver.options.get("assume_pure", False) or getattr(base, "tsde_assume_pure", False))
    counters = {} if assume_pure else graph.call_counters(base)
    if counters and not keep_counters:
        return None
    book = None
    if create:
        try:
            book = base.__dict__.setdefault(ATTR, {"refused": {}, "trusted": {}})
        except AttributeError:
            return None
    return Ledger(solver, chain, base, assume_pure, counters, who, book)


class Ledger:
    """One route's view of one SDE object's book during one solve."""

    def __init__(self, solver, chain, base, assume_pure, counters, who, book):
        self.chain, self.base, self.counters = chain, base, counters
        self._assume_pure, self._book, self._state = assume_pure, book, _UNTAKEN
        self._solver_name, self._sde_type = type(solver).__name__, solver.sde.sde_type
        self._who = who or self._solver_name

    @property
    def book(self):
        if self._book is None:          # (opened with create=False: a verifying solve may have made it since)
            self._book = getattr(self.base, ATTR, None)
        return self._book

    # ---- refusals: keyed by the object's Python-side state ----------------------------------------------------------
    def _fingerprint(self):
        return ("assumed pure",) if self._assume_pure else graph.python_state(self.base, ignore=frozenset(self.counters))

    def state(self):
        """The fingerprint of the object's Python-side state, taken at most once per solve: it costs ~0.8 ms, so only when
        there is a refusal to look up or to file."""
        if self._state is _UNTAKEN:
            self._state = self._fingerprint()
        return self._state

    def refused(self):
        """Whether this solve was refused before (or its state cannot be fingerprinted). No fingerprint while nothing is."""
        if self.book is None or not self.book["refused"]:
            return False
        state = self.state()
        return state is None or (state, self.chain, self._who) in self.book["refused"]

    def refuse(self, reason):
        """File `reason` under this solve's state (the 16 most recent) and return None: the route stays stepwise."""
        state = self.state()
        if state is not None:
            refused = self.book["refused"]
            if len(refused) >= 16:
                refused.clear()
            refused[(state, self.chain, self._who)] = reason
        return None

    # ---- the side-effect check of a verifying solve --------------------------------------------------------------------
    def snapshot(self, device):
        """Python-side state and random generators before the route calls the user's code once more."""
        state = self._fingerprint()
        if self._state is _UNTAKEN:
            self._state = state
        return state, rng_states(device)

    def side_effect(self, snapshot, device):
        """Why the calls since `snapshot` disqualify the code, or None when they left state and generators alone."""
        state, rngs = snapshot
        if state is None or self._fingerprint() != state:
            return "calling f and g changes the object's Python-side state"
        if any(not torch.equal(a, b) for a, b in zip(rngs, rng_states(device))):
            return "calling f and g advances a random number generator"
        return None

    # ---- verdicts: keyed by the form --------------------------------------------------------------------------------
    def key(self, found, y0, *tags):
        # The batch size is part of the key: the interpretation runs on a probe of a few rows, so whatever the user's code
        # derives from `y.shape[0]` (`-y if y.shape[0] > 1000 else -2 * y`) is evaluated for the probe; the both-routes
        # comparison that earns the trust therefore has to be made at every batch size the form is solved at.
        return (found.structure(), self.chain, self._solver_name, self._sde_type, y0.shape[1], y0.dtype, y0.shape[0]) + tags

    def recorded(self, key):
        """The verdict filed under `key`: True, a reason, or None (never verified)."""
        return None if self.book is None else self.book["trusted"].get(key)

    def verdict(self, key):
        """(verdict, reverify) of this solve of `key`. TSDE_VERIFY_EVERY=N (or `solvers.VERIFY_EVERY`): every N-th solve of a
        trusted form runs both routes again and compares (values, and gradients where autograd records) -- a mis-recognition
        fails loudly in CI instead of quietly in training; that solve reads verdict None and reverify True. 0 (the default):
        only the first solve verifies."""
        from .solvers import VERIFY_EVERY            # (read at every solve: the switch may be set after import)
        verdict = self.book["trusted"].get(key)
        if verdict is True and VERIFY_EVERY > 0:
            solves = self.book.setdefault("solves", {})
            solves[key] = solves.get(key, 0) + 1
            if solves[key] % VERIFY_EVERY == 0:
                return None, True
        return verdict, False

    def file(self, key, verdict, reverify=False, counter_rate=None):
        """File the verdict of a verifying solve (the 32 most recent, with their counter rates and solve counts); a trusted
        form that fails its re-verification raises."""
        trusted = self.book["trusted"]
        if len(trusted) >= 32:
            trusted.clear()
            self.book.get("counter_rate", {}).clear()
            self.book.get("solves", {}).clear()
            self.book.get("kernel", {}).clear()
        trusted[key] = verdict
        if reverify and verdict is not True:
            # TSDE_VERIFY_EVERY: a form that had earned trust and no longer reproduces the stepwise solve is a loud failure
            raise RuntimeError(f"torchsde_amd: periodic re-verification (TSDE_VERIFY_EVERY) of a trusted kernel route failed: "
                               f"{verdict}. Results of earlier solves of this object on that route are suspect; "
                               "options={'trajectory_kernel': False} keeps the stepwise path.")
        if counter_rate:
            self.book.setdefault("counter_rate", {})[key] = counter_rate

    def name_kernel(self, key, name):
        """The C entry point a form's solves launch, for `describe`."""
        self.book.setdefault("kernel", {})[key] = name

    def counter_rate(self, key):
        """{call counter: advance per step} learnt by the verifying solve of `key`, or None."""
        return self.book.get("counter_rate", {}).get(key)

    def remembers(self, finding):
        """Whether this code was found to be `finding` ("program", "uses_t", "not_rows" or "rows_general") by this scheme before."""
        return self.book.get(finding) == (self.chain, self._solver_name)

    def remember(self, finding):
        self.book[finding] = (self.chain, self._solver_name)

    def note_autograd(self, reason):
        """Why this scheme's solves of the object stay stepwise while autograd records (None: no reason any more). Kept apart
        from "refused": the forward route, under no_grad, may well hold the same code."""
        notes = self.book.setdefault("autograd", {})
        if reason is None:
            notes.pop((self.chain, self._solver_name), None)
        else:
            notes[(self.chain, self._solver_name)] = reason


def book_of(sde):
    """The book of the SDE object under `sde`'s wrappers, or None."""
    while hasattr(sde, "_base_sde"):
        sde = sde._base_sde
    return getattr(sde, ATTR, None)


def describe(sde):
    """What the recognised route has decided about `sde` so far, one line per form / refusal: the answer to "why is my
    solve (not) one kernel launch?" (cf. `graph.describe_cache` for the stepwise route's launch graphs)."""
    book = book_of(sde)
    if not book:
        return ["nothing recorded: no solve of this object has reached the recognised route (see the conditions in "
                "solvers.BaseSDESolver._integrate_recognised: diagonal noise, fixed step, this package's BrownianInterval, "
                "a CUDA state of at least 8 rows)"]
    lines = []
    for key, verdict in book["trusted"].items():
        structure, _, solver, sde_type, d, dtype, batch = key[:7]
        kind = ("perceptron drift" if structure[0][0] == "perceptron"
                else f"expression program, {structure[0][1]} noise" if structure[0][0] == "program"
                else f"row-coupled system of {structure[0][1]} channels" if structure[0][0] == "rows"
                else f"row-coupled system of {structure[0][1]} channels, {structure[0][2]} Brownian channels"
                if structure[0][0] == "rows_general"
                else f"f: {structure[0][0]}, g: {structure[1][0]}")
        timed = any("table" in part for part in structure if isinstance(part, tuple))
        route = ("trajectory kernel" + (" with per-stage-time coefficient rows" if timed else "")
                 + (" (sensitivity kernel: autograd)" if key[7:] == ("autograd",) else "")
                 + (" (generated tangent unit: autograd, "
                    f"{len(set(s for s in key[8] if s >= 0)) + (structure[0][1] if key[9] else 0)} tangents per row)"
                    if structure[0][0] == "rows" and key[7:8] == ("autograd",) else "")
                 + (f" ({book['kernel'][key]})" if key in book.get("kernel", {}) else "")
                 + (" (derivative-free Milstein)" if "grad_free" in key[7:] else ""))
        lines.append(f"[{solver}, {sde_type}, batch = {batch}, d = {d}, {dtype}] {kind}: "
                     + (route if verdict is True else f"stays stepwise: {verdict}"))
    for (_, _, solver), reason in book["refused"].items():
        lines.append(f"[{solver}] stays stepwise: {reason}")
    for (_, solver), reason in book.get("autograd", {}).items():
        lines.append(f"[{solver}] with autograd recording stays stepwise: {reason}")
    return lines
