"""Small ROW-COUPLED systems -- channels that read each other -- as one trajectory-kernel launch.

The hand-written SDEs of the reference's examples are not all elementwise: `StochasticLorenz`
(examples/latent_sde_lorenz.py:56-86) splits the state into its columns, does arithmetic among them and concatenates the result

    x1, x2, x3 = torch.split(y, (1, 1, 1), dim=1)
    f1 = a1 * (x2 - x1);  f2 = a2 * x1 - x2 - x1 * x3;  f3 = x1 * x2 - a3 * x3
    return torch.cat([f1, f2, f3], dim=1)

-- and so do Van der Pol, FitzHugh-Nagumo, SIR ... The elementwise interpreters of recognise.py end at the `split`. This one
follows COLUMNS: every value derived from the state is a list of per-column expression trees over the d state channels, t and
scalar constants; `split` / `chunk` / `unbind` / `y[:, c]` / `y[:, a:b]` pick columns, + - * /, integer powers and the unary
functions act column by column, `cat` / `stack` along dim 1 assemble the result. What comes out is d scalar expressions for the
drift and d for the diffusion (diagonal noise), which torchsde_amd/specialise.py turns into a model for the program kernel with
W = d: ONE LANE OWNS A WHOLE ROW of the batch (d <= 8 state values in registers) for the whole solve. There is no interpreter
for such systems: the route exists once the generated unit is compiled (4 s, in the background; until then the solve is
stepwise), and is trusted like every recognised route only after its first solve reproduced the stepwise one.

Schemes: those of the program kernel that need no derivative of g -- Euler, midpoint, Heun, Euler-Heun, SRK.

With autograd recording (`recognise_rows(..., differentiable=True)`, solvers._integrate_rows_with_grad) the same interpretation
runs under `enable_grad` on a probe that requires grad, and every scalar constant remembers the tensor the user's code handed to
its operator: `RecognisedRows.sources`, `.trainable`, `.slots()`. specialise.source_rows_sens then generates the same statements
on scalars with tangents, and the launch writes the path-wise sensitivities of every output (kernels._RowsTrajectoryFn).

General, scalar and additive noise (`recognise_rows(..., m=m)`): the diffusion is a MATRIX (rows, d, m). The interpreter then
follows a third kind of value, (rows, a, b) kept as a * b expressions row-major -- `stack` of column lists and `cat` of
matrices along dim 1 or 2, `unsqueeze`, `reshape` of (rows, a * b) columns, `diag_embed`, `zeros_like` / `new_zeros` ...
(literal constants), `expand` / `repeat` of a state-independent (d, m) tensor or of a (d, m) function of t (one live scalar
constant per entry) and the arithmetic above entry by entry. `RecognisedRows.outputs` holds the d drift expressions and the
d * m entries; an entry that is the literal 0 is structural (`zero_mask`), and specialise.source_rows_general emits the
contraction with the row's m increments without a term for it (csrc/trajectory.hip trajectory_rows_general_kernel: Euler,
midpoint, Heun, Euler-Heun, values only).
"""
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from .recognise import NotElementwise, _Expr

MAX_D = 8
_UNARY = {"exp", "log", "sin", "cos", "tanh", "sigmoid", "sqrt", "abs", "relu", "reciprocal", "neg"}
_VIEWS = {"alias", "detach", "clone", "contiguous", "lift_fresh", "positive", "_to_copy"}


def _const(value):
    return _Expr("const", value=value)


class _Columns(TorchDispatchMode):
    """`cols[id(tensor)]`: the column expressions of a (rows, k) or (rows,) value derived from the state -- or, a third kind
    (`mats`), the a * b entries of a MATRIX (rows, a, b), row-major: the diffusion of general, scalar and additive noise."""

    def __init__(self, y, t, rows, d, matrix=False):
        super().__init__()
        self.rows, self.d = rows, d
        self.matrix = bool(matrix)  # `recognise_rows(..., m=m)`: matrices are followed; False: exactly the two kinds above
        self.cols = {id(y): [_Expr("y", value=c) for c in range(d)]}
        self.keep = [y, t]
        self.t_id = id(t)
        self.flat = set()           # ids of tracked values of shape (rows,) (a column without its unit axis)
        self.scalar_like = set()    # ids of 0-d functions of t (they broadcast against either kind)
        self.mats = {}              # id of a tracked matrix -> (a, b); its a * b entries row-major in `cols`
        self.free = set()           # ids of tracked matrices WITHOUT the batch axis, (a, b) or (1, a, b): functions of t alone
        self.literal = {}           # id of a state-independent tensor filled with one number (`zeros`, `ones`, `full`) -> it
        self.shape = None           # (a, b) while `elementwise` works on matrix entries (`columns_of`)
        self.made = {id(y), id(t)}  # ids of tensors whose storage was allocated during the interpretation
        self.differentiable = False # True: the kernel's GRADIENTS will stand for autograd through this code (recognise_rows)
        self.sources = {}           # differentiable: id(a scalar constant) -> (the operand the code handed over, flat index)

    def track(self, tensor, cols, flat=False, mat=None):
        want = (self.rows,) + tuple(mat) if mat else ((self.rows,) if flat else (self.rows, len(cols)))
        if tuple(tensor.shape) != want or (mat and mat[0] * mat[1] != len(cols)):
            raise NotElementwise(f"a value derived from the state has shape {tuple(tensor.shape)}, not {want}")
        self.cols[id(tensor)] = list(cols)
        if flat:
            self.flat.add(id(tensor))
        if mat:
            self.mats[id(tensor)] = tuple(mat)
        self.keep.append(tensor)
        return tensor

    def track_by_shape(self, tensor, cols, what):
        """`tensor` keeps the batch axis first and its `cols` in row-major order: flat, columns or a matrix by its shape."""
        shape = tuple(tensor.shape)
        if not shape or shape[0] != self.rows or len(shape) > 3:
            raise NotElementwise(f"{what} gives a value derived from the state shape {shape}")
        if len(shape) == 3:
            return self.track(tensor, cols, mat=shape[1:])
        return self.track(tensor, cols, flat=len(shape) == 1)

    def entries_of(self, x, a, b):
        """The a * b entries, row-major, of operand x beside a matrix: a tracked matrix of that shape or one that broadcasts
        -- (rows, a, 1) against (rows, 1, b) --, t, a number, or a state-independent tensor that broadcasts over the batch
        (one scalar constant per entry: its live value at every launch)."""
        def spread(entries, sa, sb):
            if (sa not in (1, a)) or (sb not in (1, b)) or len(entries) != sa * sb:
                raise NotElementwise(f"an operand of shape {(sa, sb)} per row beside a matrix of shape {(a, b)} per row")
            return [entries[(i if sa > 1 else 0) * sb + (k if sb > 1 else 0)] for i in range(a) for k in range(b)]
        if torch.is_tensor(x) and id(x) in self.cols:
            if id(x) in self.mats:
                return spread(self.cols[id(x)], *self.mats[id(x)])
            if id(x) in self.scalar_like:
                return self.cols[id(x)] * (a * b)
            raise NotElementwise("columns of the state and a matrix in one operation")
        if torch.is_tensor(x) and id(x) == self.t_id:
            return [_Expr("t")] * (a * b)
        if isinstance(x, (bool, int, float)):
            return [_const(float(x))] * (a * b)
        if torch.is_tensor(x):
            if id(x) in self.literal:
                return [_const(self.literal_value(x))] * (a * b)
            if x.numel() == 1:
                return [self.scalar_of(x, x.reshape(()), 0)] * (a * b)
            shape = tuple(x.shape)
            if len(shape) == 3 and shape[0] == 1:
                shape = shape[1:]
            if len(shape) > 2:
                raise NotElementwise(f"an operand of shape {tuple(x.shape)} beside a matrix derived from the state "
                                     "(a per-row constant?)")
            shape = (1,) * (2 - len(shape)) + shape
            flat = x.reshape(-1)
            return spread([self.scalar_of(x, flat[j], j) for j in range(flat.numel())], *shape)
        raise NotElementwise(f"an operand of type {type(x).__name__}")

    def literal_value(self, x):
        """The number a `zeros` / `ones` / `full` tensor was filled with -- if it still holds it everywhere."""
        value = self.literal[id(x)]
        if not bool((x == value).all()):
            raise NotElementwise("a tensor made with zeros / ones / full was written into afterwards")
        return float(value)

    def untracked(self, name, args, kwargs, out):
        """What an operation on state-independent tensors leaves to remember: tensors filled with one number are literal
        constants; `expand` / `repeat` of a tensor without a batch axis to (rows, a, b) is a matrix whose every row is that
        tensor -- one constant per entry."""
        if not torch.is_tensor(out):
            return out
        src = args[0] if args and torch.is_tensor(args[0]) else None
        if name in ("zeros", "ones", "full", "zeros_like", "ones_like", "full_like", "new_zeros", "new_ones", "new_full"):
            fill = kwargs.get("fill_value", args[-1] if "full" in name else None)
            value = 0.0 if "zeros" in name else (1.0 if "ones" in name else fill)
            if isinstance(value, (bool, int, float)):
                self.literal[id(out)] = float(value)
                self.keep.append(out)
        elif src is not None and id(src) in self.literal and name in _VIEWS | {"expand", "repeat", "view", "reshape",
                                                                                "_unsafe_view", "unsqueeze", "squeeze"}:
            self.literal[id(out)] = self.literal[id(src)]
            self.keep.append(out)
        elif name in ("expand", "repeat") and src is not None and out.dim() == 3 and out.shape[0] == self.rows \
                and (src.dim() < 3 or src.shape[0] == 1):
            if name == "repeat" and tuple(out.shape[1:]) != tuple(((1, 1) + tuple(src.shape))[-2:]):
                return out                       # (tiled along the channels: not followed)
            return self.track(out, self.entries_of(src, out.shape[1], out.shape[2]), mat=tuple(out.shape[1:]))
        return out

    def columns_of(self, x, k):
        """The k column expressions of operand x: a tracked value (k columns, or one that broadcasts), t, or a constant."""
        if self.shape is not None:
            return self.entries_of(x, *self.shape)
        if torch.is_tensor(x) and id(x) in self.mats:
            raise NotElementwise("columns of the state and a matrix in one operation")
        if torch.is_tensor(x) and id(x) in self.cols:
            c = self.cols[id(x)]
            if len(c) == k:
                return c
            if len(c) == 1:
                return c * k
            raise NotElementwise("operands with different numbers of columns")
        if torch.is_tensor(x) and id(x) == self.t_id:
            return [_Expr("t")] * k
        if isinstance(x, (bool, int, float)):
            return [_const(float(x))] * k
        if torch.is_tensor(x):
            if x.numel() == 1:
                return [self.scalar_of(x, x.reshape(()), 0)] * k
            if x.dim() <= 2 and x.shape[-1] == k and x.numel() == k:
                flat = x.reshape(-1)
                return [self.scalar_of(x, flat[j], j) for j in range(k)]
            raise NotElementwise(f"an operand of shape {tuple(x.shape)} beside columns of the state")
        raise NotElementwise(f"an operand of type {type(x).__name__}")

    def scalar_of(self, x, element, j):
        """The constant `element` = element j of operand x. The slice is made below autograd and carries no graph; the
        differentiable interpretation therefore remembers the operand itself -- a parameter, or what autograd saw the code
        derive from parameters -- which still has its `grad_fn` here."""
        if self.differentiable:
            self.sources[id(element)] = (x, j)
        return _const(element)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        self.check_side_effects(func, args, kwargs)
        out = self.follow(func, args, kwargs)
        returns = func._schema.returns
        outs = out if isinstance(out, (list, tuple)) else (out,)
        for k, o in enumerate(outs):
            if torch.is_tensor(o) and id(o) not in self.made:
                aliasing = k < len(returns) and returns[k].alias_info is not None
                if not aliasing or (args and torch.is_tensor(args[0]) and id(args[0]) in self.made):
                    self.made.add(id(o))
                    self.keep.append(o)
        return out

    def check_side_effects(self, func, args, kwargs):
        """As recognise._Interpreter.check_side_effects: the code runs once per solve here, once per step in the reference
        (base_solver.py:114-149) -- random draws and in-place writes to tensors that existed before the call end the
        interpretation."""
        schema = func._schema
        if torch.Tag.nondeterministic_seeded in func.tags:
            raise NotElementwise(f"{schema.name} draws random numbers: once per solve here, once per step in the reference")
        if not schema.is_mutable:
            return
        for i, arg in enumerate(schema.arguments):
            if arg.alias_info is None or not arg.alias_info.is_write:
                continue
            value = args[i] if i < len(args) else kwargs.get(arg.name)
            for x in (value if isinstance(value, (list, tuple)) else (value,)):
                if torch.is_tensor(x) and id(x) not in self.made:
                    raise NotElementwise(f"in-place {schema.name} on a tensor that existed before f and g were called "
                                         "(state that outlives the call: once per solve here, once per step in the reference)")

    def follow(self, func, args, kwargs):
        schema = func._schema
        name = schema.name.split("::")[1]
        flat_args = list(args) + list(kwargs.values())
        tensors = [a for a in flat_args if torch.is_tensor(a)]
        for a in flat_args:
            if isinstance(a, (list, tuple)):
                tensors.extend(x for x in a if torch.is_tensor(x))
        for a in tensors:
            self.keep.append(a)
        tracked = [a for a in tensors if id(a) in self.cols]
        if self.differentiable:
            for a in tracked:
                if a.is_floating_point() and not a.requires_grad and any(c.mentions_state() for c in self.cols[id(a)]):
                    raise NotElementwise("a stop-gradient on a value derived from the state")
        uses_t = any(id(a) == self.t_id for a in tensors)
        if not tracked and not uses_t:
            out = func(*args, **kwargs)
            return self.untracked(name, args, kwargs, out) if self.matrix else out
        if uses_t and not tracked:
            if name in ("_local_scalar_dense", "item"):
                raise NotElementwise("the code reads t on the host")
            # arithmetic among t and constants: a (0-d) function of t, followed as a one-column value
            out = func(*args, **kwargs)
            if self.matrix and torch.is_tensor(out) and out.numel() != 1 and out.dim() in (2, 3):
                return self.matrix_arithmetic(name, args, kwargs, out, [])     # t beside a (d, m) tensor: a matrix function of t
            if not torch.is_tensor(out) or out.numel() != 1:
                raise NotElementwise(f"{name} makes something other than a number out of t")
            expr = self.elementwise(name, args, kwargs, 1, out)
            self.cols[id(out)] = expr
            self.keep.append(out)
            self.scalar_like.add(id(out))
            return out
        if schema.is_mutable:
            raise NotElementwise(f"in-place {name} on a value derived from the state")
        out = func(*args, **kwargs)
        src = args[0] if args and torch.is_tensor(args[0]) and id(args[0]) in self.cols else None
        if src is not None and id(src) in self.free:
            # a matrix function of t, no batch axis yet: `expand` / `repeat` give it one, every row the same entries
            a, b = self.mats[id(src)]
            if name in ("expand", "repeat") and out.dim() == 3 and out.shape[0] == self.rows and (
                    name == "expand" or tuple(out.shape[1:]) == (a, b)):
                return self.track(out, self.entries_of(src, out.shape[1], out.shape[2]), mat=tuple(out.shape[1:]))
            if (name in _VIEWS or name in ("unsqueeze", "squeeze", "view", "reshape")) and tuple(out.shape) in ((a, b), (1, a, b)):
                return self.track_free(out, self.cols[id(src)], (a, b))
            raise NotElementwise(f"operator {name} on a matrix function of t")
        if name in _VIEWS and src is not None and torch.is_tensor(out) and out.shape == src.shape and out.dtype == src.dtype:
            return self.track(out, self.cols[id(src)], flat=id(src) in self.flat, mat=self.mats.get(id(src)))
        if src is not None and id(src) in self.mats and name in ("split_with_sizes", "split", "chunk", "unbind", "tensor_split",
                                                                 "select", "slice", "narrow"):
            raise NotElementwise(f"operator {name} on a matrix derived from the state")
        if name in ("split_with_sizes", "split", "chunk", "unbind", "tensor_split") and src is not None:
            dim = args[2] if len(args) > 2 else kwargs.get("dim", 0)
            if name == "unbind":
                dim = args[1] if len(args) > 1 else kwargs.get("dim", 0)
            if id(src) in self.flat or dim not in (1, -1):
                raise NotElementwise(f"{name} of the state along the batch")
            cols, at, pieces = self.cols[id(src)], 0, []
            for piece in out:
                if name == "unbind":
                    pieces.append(self.track(piece, cols[at:at + 1], flat=True))
                    at += 1
                else:
                    width = piece.shape[1]
                    pieces.append(self.track(piece, cols[at:at + width]))
                    at += width
            return type(out)(pieces) if isinstance(out, tuple) else pieces
        if name == "select" and src is not None and id(src) not in self.flat:
            dim, index = args[1], args[2]
            if dim not in (1, -1):
                raise NotElementwise("a row of the batch is picked out")
            return self.track(out, [self.cols[id(src)][index]], flat=True)
        if name in ("slice", "narrow") and src is not None:
            dim = args[1] if len(args) > 1 else kwargs.get("dim", 0)
            if dim in (1, -1) and id(src) not in self.flat:
                cols = self.cols[id(src)]
                if name == "slice":
                    start = args[2] if len(args) > 2 and args[2] is not None else 0
                    end = args[3] if len(args) > 3 and args[3] is not None else len(cols)
                    step = args[4] if len(args) > 4 else 1
                    picked = cols[slice(start, min(end, len(cols)), step)]
                else:
                    picked = cols[args[2]:args[2] + args[3]]
                return self.track(out, picked)
            if tuple(out.shape) == tuple(src.shape):           # `y[:]`: the whole batch
                return self.track(out, self.cols[id(src)], flat=id(src) in self.flat)
            raise NotElementwise("rows of the batch are picked out")
        if name in ("unsqueeze", "squeeze", "view", "reshape", "_unsafe_view", "_reshape_alias") and src is not None:
            cols = self.cols[id(src)]
            if tuple(out.shape) == (self.rows, len(cols)):
                return self.track(out, cols)
            if len(cols) == 1 and tuple(out.shape) == (self.rows,):
                return self.track(out, cols, flat=True)
            if self.matrix and out.dim() == 3 and out.shape[0] == self.rows and not (name == "unsqueeze" and args[1] in (0, -out.dim())):
                # (rows, a * b) -> (rows, a, b), (rows, k) -> (rows, k, 1) or (rows, 1, k): the batch axis stays in front, the
                # row's values keep their row-major order
                return self.track(out, cols, mat=tuple(out.shape[1:]))
            raise NotElementwise(f"{name} gives a value derived from the state shape {tuple(out.shape)}")
        if self.matrix and name == "diag_embed" and src is not None and id(src) not in self.flat and id(src) not in self.mats:
            if tuple(args[1:]) not in ((), (0,), (0, -2), (0, -2, -1)) or any(
                    kwargs.get(key, value) != value for key, value in (("offset", 0), ("dim1", -2), ("dim2", -1))):
                raise NotElementwise("diag_embed with an offset or other axes")
            cols = self.cols[id(src)]
            k = len(cols)
            return self.track(out, [cols[i] if i == j else _const(0.0) for i in range(k) for j in range(k)], mat=(k, k))
        if self.matrix and name in ("cat", "stack") and self.assembles_matrix(name, args[0]):
            return self.assemble_matrix(name, args[0], args[1] if len(args) > 1 else kwargs.get("dim", 0), out)
        if name in ("cat", "stack"):
            pieces = args[0]
            dim = args[1] if len(args) > 1 else kwargs.get("dim", 0)
            if dim not in (1, -1):
                raise NotElementwise(f"{name} along the batch")
            cols = []
            for piece in pieces:
                if id(piece) not in self.cols or id(piece) in self.scalar_like:
                    raise NotElementwise(f"{name} with a block that is not made of columns of the state")
                if (name == "stack") != (id(piece) in self.flat):
                    raise NotElementwise(f"{name} of columns with / without their unit axis")
                cols.extend(self.cols[id(piece)])
            return self.track(out, cols)
        if name in ("zeros_like", "ones_like") and src is not None:
            value = 0.0 if name == "zeros_like" else 1.0
            if id(src) not in self.mats:
                return self.track(out, [_const(value)] * len(self.cols[id(src)]), flat=id(src) in self.flat)
        if self.matrix and name in ("zeros_like", "ones_like", "full_like", "new_zeros", "new_ones", "new_full") \
                and src is not None:
            # literal constants in the shape asked for: a zero entry of a diffusion matrix is STRUCTURAL (`RecognisedRows.zero_mask`)
            fill = kwargs.get("fill_value", args[-1] if "full" in name else None)
            value = 0.0 if "zeros" in name else (1.0 if "ones" in name else fill)
            if not isinstance(value, (bool, int, float)):
                raise NotElementwise(f"{name} with a fill value that is not a number")
            if out.dim() and out.shape[0] == self.rows and id(src) not in self.free:
                return self.track_by_shape(out, [_const(float(value))] * (out.numel() // self.rows), name)
            self.literal[id(out)] = float(value)
            self.keep.append(out)
            return out
        # elementwise arithmetic, column by column
        shaped = [a for a in tracked if id(a) not in self.scalar_like]
        if any(id(a) in self.mats for a in shaped) or (self.matrix and not shaped and torch.is_tensor(out) and out.numel() != 1
                                                      and out.dim() in (2, 3)):
            return self.matrix_arithmetic(name, args, kwargs, out, shaped)
        if not shaped:               # functions of t among themselves
            expr = self.elementwise(name, args, kwargs, 1, out)
            self.cols[id(out)] = expr
            self.keep.append(out)
            self.scalar_like.add(id(out))
            return out
        k = max(len(self.cols[id(a)]) for a in shaped)
        flat = all(id(a) in self.flat for a in shaped)
        if any((id(a) in self.flat) != flat for a in shaped):
            raise NotElementwise("columns with and without their unit axis in one operation")
        return self.track(out, self.elementwise(name, args, kwargs, k, out), flat=flat)

    def track_free(self, tensor, entries, shape):
        """A matrix function of t without a batch axis, (a, b) or (1, a, b)."""
        self.cols[id(tensor)] = list(entries)
        self.mats[id(tensor)] = tuple(shape)
        self.free.add(id(tensor))
        self.keep.append(tensor)
        return tensor

    def matrix_arithmetic(self, name, args, kwargs, out, shaped):
        """The unary and binary tables entry by entry: between matrices of one shape (or (rows, d, 1) against (., 1, m)), and
        between a matrix and a number, a function of t or a state-independent tensor that broadcasts over the batch
        (`entries_of`). Without any operand that has a batch axis the result has none either (`free`)."""
        for a in shaped:
            if id(a) not in self.mats:
                raise NotElementwise("columns of the state and a matrix in one operation")
        free = all(id(a) in self.free for a in shaped)
        shape = tuple(out.shape) if torch.is_tensor(out) else ()
        if free and len(shape) == 3 and shape[0] == 1:
            shape = shape[1:]
        if len(shape) != (2 if free else 3) or (not free and shape[0] != self.rows):
            raise NotElementwise(f"{name} gives a matrix derived from the state or t shape {tuple(shape)}")
        shape = shape[-2:]
        self.shape = shape
        try:
            entries = self.elementwise(name, args, kwargs, shape[0] * shape[1], out)
        finally:
            self.shape = None
        return self.track_free(out, entries, shape) if free else self.track(out, entries, mat=shape)

    def piece_of_matrix(self, piece, dims):
        """(entries, per-row shape) of a block of `cat` / `stack`: a tracked value with a batch axis and `dims` axes, or a
        tensor of that shape made with zeros / ones / full."""
        if torch.is_tensor(piece) and piece.dim() == dims and piece.shape[0] == self.rows:
            shape = tuple(piece.shape[1:])
            if id(piece) in self.literal:
                count = shape[0] * (shape[1] if dims == 3 else 1)
                return [_const(self.literal_value(piece))] * count, shape
            if (id(piece) in self.cols and id(piece) not in self.scalar_like and id(piece) not in self.free
                    and id(piece) not in self.flat and (id(piece) in self.mats) == (dims == 3)):
                return self.cols[id(piece)], shape
        raise NotElementwise("a block that is neither made from the state nor a batch-independent constant (a per-row constant?)")

    def assembles_matrix(self, name, pieces):
        """Whether this `cat` / `stack` builds a matrix: `stack` of column lists (rows, k), `cat` of matrices."""
        tracked = [p for p in pieces if torch.is_tensor(p) and id(p) in self.cols and id(p) not in self.scalar_like]
        if name == "cat":
            return any(id(p) in self.mats for p in tracked)
        return bool(tracked) and all(id(p) not in self.flat and id(p) not in self.mats for p in tracked)

    def assemble_matrix(self, name, pieces, dim, out):
        dim = dim + 3 if dim < 0 else dim
        if dim not in (1, 2):
            raise NotElementwise(f"{name} along the batch")
        blocks = [self.piece_of_matrix(p, 3 if name == "cat" else 2) for p in pieces]
        if name == "stack":              # n column lists of k: (rows, n, k) along dim 1, (rows, k, n) along dim 2
            blocks = [(e, (1, s[0]) if dim == 1 else (s[0], 1)) for e, s in blocks]
        if dim == 1:
            if len({s[1] for _, s in blocks}) != 1:
                raise NotElementwise(f"{name} of blocks of different widths")
            entries = [x for e, _ in blocks for x in e]
            shape = (sum(s[0] for _, s in blocks), blocks[0][1][1])
        else:
            if len({s[0] for _, s in blocks}) != 1:
                raise NotElementwise(f"{name} of blocks of different heights")
            a = blocks[0][1][0]
            entries = [x for i in range(a) for e, s in blocks for x in e[i * s[1]:(i + 1) * s[1]]]
            shape = (a, sum(s[1] for _, s in blocks))
        return self.track(out, entries, mat=shape)

    def elementwise(self, name, args, kwargs, k, out):
        if name in ("clamp", "clamp_min") and self.differentiable:
            # (as the program route, recognise.py: torch's clamp passes the gradient AT the boundary, the kernels' relu does not)
            raise NotElementwise("clamp with autograd recording: its backward passes the gradient at the boundary, relu's does not")
        if name in _UNARY and len(args) == 1:
            return [_Expr(name, (c,)) for c in self.columns_of(args[0], k)]
        if name == "softplus":
            beta = args[1] if len(args) > 1 else kwargs.get("beta", 1)
            threshold = args[2] if len(args) > 2 else kwargs.get("threshold", 20)
            if beta != 1 or threshold != 20:
                raise NotElementwise("softplus with a non-default beta or threshold")
            return [_Expr("softplus", (c,)) for c in self.columns_of(args[0], k)]
        if name == "pow" and len(args) == 2 and isinstance(args[1], (int, float)):
            n = args[1]
            table = {1: None, 2: "square", 3: "cube", 0.5: "sqrt", -1: "reciprocal"}
            if n not in table:
                raise NotElementwise(f"the power {n}")
            cols = self.columns_of(args[0], k)
            return cols if table[n] is None else [_Expr(table[n], (c,)) for c in cols]
        if name in ("mul", "add", "sub", "rsub", "div") and len(args) >= 2:
            for key, value in kwargs.items():
                if key != "alpha" and value is not None:
                    raise NotElementwise(f"{name} with {key}={value!r}")
            a, b = self.columns_of(args[0], k), self.columns_of(args[1], k)
            alpha = kwargs.get("alpha", 1)
            if name == "rsub":
                a, b, name = b, a, "sub"
            if alpha != 1:
                if not isinstance(alpha, (int, float)):
                    raise NotElementwise("a tensor-valued alpha")
                b = [_Expr("mul", (c, _const(float(alpha)))) for c in b]
            return [_Expr(name, (x, y)) for x, y in zip(a, b)]
        raise NotElementwise(f"operator {name} on columns of the state")


class RecognisedRows:
    """d drift and d diffusion expressions over the row's d channels, t and scalar constants -- or (`m`: general, scalar and
    additive noise) d drift expressions and the d * m entries of the diffusion matrix, row-major."""
    perceptron = neural = timed = False
    exact = False

    def __init__(self, f, g, d, dtype, device, sources=None, m=None):
        self.f, self.g, self.d, self.dtype, self.device = list(f), list(g), d, dtype, device
        self.m = m
        # entries of the diffusion matrix that are the literal 0 are STRUCTURAL: the generated contraction has no term for them
        self.zero_mask = None if m is None else tuple(
            e.op == "const" and not torch.is_tensor(e.value) and float(e.value) == 0.0 for e in self.g)
        self.consts = []            # scalar constants in order of first use: numbers, or 0-d tensors (live values)
        self.statements, self.outputs = self._linearise()
        # the differentiable interpretation (`recognise_rows(..., differentiable=True)`): where the constants come from
        self.sources = []           # the distinct operand tensors with requires_grad that constants were taken from
        self.trainable = []         # the trainable scalars, in tangent-slot order: (index into `sources`, flat element index)
        self.const_slot = {}        # index into `consts` -> index into `trainable`
        self.untrainable = None     # why the constants cannot carry gradients, if they cannot
        for k, c in enumerate(self.consts):
            x, j = (sources or {}).get(id(c), (None, 0))
            if x is None or not x.requires_grad:
                continue
            if not x.is_floating_point() or x.dtype != dtype or x.device != device:
                self.untrainable = f"a trainable constant of dtype {x.dtype} on {x.device} beside a state of {dtype} on {device}"
                continue
            for s, have in enumerate(self.sources):
                if have is x:
                    break
            else:
                self.sources.append(x)
                s = len(self.sources) - 1
            if (s, j) not in self.trainable:
                self.trainable.append((s, j))
            self.const_slot[k] = self.trainable.index((s, j))

    def _linearise(self):
        """Every distinct node once, in evaluation order: [(name, op, operand names)], and the 2 d output names."""
        names, statements = {}, []

        def visit(node):
            if id(node) in names:
                return names[id(node)]
            if node.op == "y":
                name = f"x.v[{node.value}]"
            elif node.op == "t":
                name = "time"
            elif node.op == "const":
                if torch.is_tensor(node.value):
                    for k, have in enumerate(self.consts):
                        if have is node.value:
                            break
                    else:
                        self.consts.append(node.value)
                        k = len(self.consts) - 1
                    name = f"c[{k}]"
                else:
                    name = f"(T){float(node.value)!r}"
            else:
                operands = [visit(a) for a in node.args]
                name = f"n{len(statements)}"
                statements.append((name, node.op, operands))
            names[id(node)] = name
            return name
        outputs = [visit(n) for n in self.f] + [visit(n) for n in self.g]
        if len(statements) > 512:
            raise NotElementwise("a system of more than 512 operations")
        return statements, outputs

    def structure(self):
        statements = tuple((op, tuple(operands)) for _, op, operands in self.statements)
        if self.m is not None:
            return (("rows_general", self.d, self.m, statements, tuple(self.outputs)), ("consts", len(self.consts)))
        return (("rows", self.d, statements, tuple(self.outputs)), ("consts", len(self.consts)))

    def affine_leaves(self):
        return None

    def const_table(self):
        if not self.consts:
            return torch.zeros(1, dtype=self.dtype, device=self.device)
        return torch.stack([c.detach().to(device=self.device, dtype=self.dtype).reshape(()) for c in self.consts]).contiguous()

    def spec(self):
        if self.m is not None:
            return ("program_rows_general", self.structure(), self.const_table(), self.d, self.m)
        return ("program_rows", self.structure(), self.const_table(), self.d)

    def slots(self):
        """Per constant its tangent slot among the trainable scalars, or -1: part of the generated tangent unit's key."""
        return tuple(self.const_slot.get(k, -1) for k in range(len(self.consts)))

    def reaches(self, params):
        """Whether every tensor of `params` that requires grad is reached through `sources` -- is one of them, or a leaf of
        the graph autograd recorded on the way to one (as solvers._integrate_program_with_grad asks of its constants): a
        parameter that is not would lose its gradient on the kernel route."""
        reached = set()
        for x in self.sources:
            stack, seen = [x.grad_fn], set()
            if x.is_leaf:
                reached.add(id(x))
            while stack:
                fn = stack.pop()
                if fn is None or id(fn) in seen:
                    continue
                seen.add(id(fn))
                if hasattr(fn, "variable"):
                    reached.add(id(fn.variable))
                stack.extend(nxt for nxt, _ in fn.next_functions)
        return all(id(p) in reached for p in params if p.requires_grad)


MAX_M = 8


def recognise_rows(sde, t, y0, rows=None, differentiable=False, m=None):
    """`RecognisedRows` for a diagonal-noise SDE whose f and g do arithmetic among the columns of the state, or NotElementwise.
    `m`: the number of Brownian channels of an SDE with general, scalar or additive noise, whose diffusion is then a
    (rows, d, m) matrix assembled from such arithmetic (values only)."""
    if m is not None:
        m = int(m)
        if differentiable:
            raise NotElementwise("no tangent unit for a diffusion matrix")
        if m < 1 or m > MAX_M:
            raise NotElementwise(f"a row-coupled system of {m} Brownian channels, more than {MAX_M}")
    rows = 2 if rows is None else int(rows)
    if rows == y0.shape[0]:
        rows += 1
    d = y0.shape[1]
    if d > MAX_D:
        raise NotElementwise(f"a row-coupled system of more than {MAX_D} channels")
    probe = y0.detach()[:1].expand(rows, d).clone() if y0.shape[0] > 0 else torch.zeros(rows, d, dtype=y0.dtype, device=y0.device)
    t_probe = t.detach().clone()
    if differentiable:
        probe.requires_grad_(True)               # (so that a stop-gradient in the user's code shows: `_Columns.follow`)
    interp = _Columns(probe, t_probe, rows, d, matrix=m is not None)
    interp.differentiable = bool(differentiable)
    try:
        # `differentiable`: autograd watches the user's own constant arithmetic, so that a constant which is derived from
        # parameters carries its graph back to them (cf. recognise.recognise_program)
        with (torch.enable_grad() if differentiable else torch.no_grad()), interp:
            f, g = sde.f_and_g(t_probe, probe)
    except NotElementwise:
        raise
    except Exception as e:
        raise NotElementwise(f"{type(e).__name__}: {e}") from None
    out = []
    for name, value in (("drift", f), ("diffusion", g)):
        cols = interp.cols.get(id(value)) if torch.is_tensor(value) else None
        if m is not None and name == "diffusion":
            if cols is None or interp.mats.get(id(value)) != (d, m) or id(value) in interp.free \
                    or tuple(value.shape) != (rows, d, m):
                shape = tuple(value.shape) if torch.is_tensor(value) else type(value).__name__
                raise NotElementwise(f"the diffusion ({shape}) is not a (rows, d, m) = ({rows}, {d}, {m}) value assembled from "
                                     "columns of the state and batch-independent constants")
            out.append(cols)
            continue
        if cols is None or id(value) in interp.flat or len(cols) != d or tuple(value.shape) != (rows, d):
            raise NotElementwise(f"the {name} is not a (rows, d) value assembled from columns of the state")
        if differentiable and not value.requires_grad and any(c.mentions_state() for c in cols):
            raise NotElementwise(f"a stop-gradient on a value derived from the state (the {name})")
        out.append(cols)
    found = RecognisedRows(out[0], out[1], d, y0.dtype, y0.device, interp.sources if differentiable else None, m=m)
    found._alive = interp.keep
    return found
