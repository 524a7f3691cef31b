"""Expression programs compiled instead of interpreted.

`tsde_trajectory_prog_diag` runs drift and diffusion of a recognised user module as postfix programs through an interpreter in
the kernel (csrc/trajectory.hip, `ProgModel`): a compare tree and register shuffles per instruction, ~3 000 cycles per
wave-step where the hand-written affine kernel needs ~400. This module turns the SAME instruction words into straight-line HIP
code -- a struct with the interpreter's interface, `f<SLOT>(x)`, `g<SLOT>(x)`, `gdg<SLOT>(x, g, v)` -- and instantiates the
interpreter's own kernel (`trajectory_prog_kernel<T, METHOD, W, Model>`: same loop, same schemes, same generator) with it,
through the interpreter's own launch helpers (csrc/trajectory.hip `prog_args`, `launch_prog_m` ...: a unit is a model, `_model`,
plus one entry point of a few lines, `_unit`):
one operation of the user's code = one statement, in the order the interpreter would execute it, with the same functions and
`-ffp-contract=off`, hence THE SAME BITS (checked on first use: the specialised launch must equal the interpreter's with
`torch.equal`, or it is never used).

The translation unit is compiled with the toolchain's `hipcc` (~4 s) in a background thread and cached by the hash of its source
under ``~/.cache/torchsde_amd/specialised/`` (``TSDE_SPECIALISE_CACHE``); until the library is there -- and whenever there is no
compiler -- the interpreter runs. ``TSDE_SPECIALISE=0`` switches the mechanism off, ``TSDE_SPECIALISE=sync`` compiles in the
calling thread (tests, benchmarks). The reference has no counterpart: its loop (base_solver.py:114-149) calls the user's Python
code at every step.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess
import threading

import torch

from . import _native

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
MODE = os.environ.get("TSDE_SPECIALISE", "1").strip().lower()          # "0" | "1" (background) | "sync"

_OPS = {0: "load", 1: "add", 2: "sub", 3: "rsub", 4: "mul", 5: "div", 6: "rdiv", 16: "neg", 17: "exp", 18: "log", 19: "sin",
        20: "cos", 21: "tanh", 22: "sigmoid", 23: "softplus", 24: "sqrt", 25: "abs", 26: "relu", 27: "reciprocal",
        28: "square", 29: "cube", 30: "dup"}
_SRC_STACK, _SRC_CONST, _SRC_STATE, _SRC_TIME = 0, 1, 2, 3
_UNARY = {
    "neg": "vmap({0}, [](T v) {{ return -v; }})", "exp": "vmap({0}, [](T v) {{ return exp(v); }})",
    "log": "vmap({0}, [](T v) {{ return log(v); }})", "sin": "vmap({0}, [](T v) {{ return sin(v); }})",
    "cos": "vmap({0}, [](T v) {{ return cos(v); }})", "tanh": "vmap({0}, [](T v) {{ return tanh(v); }})",
    "sigmoid": "vmap({0}, [](T v) {{ return (T)1 / ((T)1 + exp(-v)); }})",
    "softplus": "vmap({0}, [](T v) {{ return v > (T)20 ? v : log1p(exp(v)); }})",
    "sqrt": "vmap({0}, [](T v) {{ return sqrt(v); }})", "abs": "vmap({0}, [](T v) {{ return fabs(v); }})",
    "relu": "vmap({0}, [](T v) {{ return v > (T)0 ? v : (T)0; }})",
    "reciprocal": "vmap({0}, [](T v) {{ return (T)1 / v; }})", "square": "({0} * {0})", "cube": "(({0} * {0}) * {0})",
}
_BINARY = {"add": "({a} + {b})", "sub": "({a} - {b})", "rsub": "({b} - {a})", "mul": "({a} * {b})", "div": "({a} / {b})",
           "rdiv": "({b} / {a})"}


# the same functions on forward-mode dual numbers: value and slope exactly as ProgSensModel::run forms them
_DUAL_HELPERS = '''
template <typename T> TSDE_D Dual<T> d_neg(const Dual<T>& s) { return chain(s, -s.v, (T)-1); }
template <typename T> TSDE_D Dual<T> d_exp(const Dual<T>& s) { const T e = exp(s.v); return chain(s, e, e); }
template <typename T> TSDE_D Dual<T> d_log(const Dual<T>& s) { return chain(s, log(s.v), (T)1 / s.v); }
template <typename T> TSDE_D Dual<T> d_sin(const Dual<T>& s) { return chain(s, sin(s.v), cos(s.v)); }
template <typename T> TSDE_D Dual<T> d_cos(const Dual<T>& s) { return chain(s, cos(s.v), -sin(s.v)); }
template <typename T> TSDE_D Dual<T> d_tanh(const Dual<T>& s) { const T t = tanh(s.v); return chain(s, t, (T)1 - t * t); }
template <typename T> TSDE_D Dual<T> d_sigmoid(const Dual<T>& s) {
  const T g = (T)1 / ((T)1 + exp(-s.v));
  return chain(s, g, g * ((T)1 - g));
}
template <typename T> TSDE_D Dual<T> d_softplus(const Dual<T>& s) {
  const T v = s.v;
  const T z = exp(v);
  return chain(s, v > (T)20 ? v : log1p(z), v > (T)20 ? (T)1 : z / (z + (T)1));
}
template <typename T> TSDE_D Dual<T> d_sqrt(const Dual<T>& s) { const T r = sqrt(s.v); return chain(s, r, (T)0.5 / r); }
template <typename T> TSDE_D Dual<T> d_abs(const Dual<T>& s) {
  const T v = s.v;
  return chain(s, fabs(v), v > (T)0 ? (T)1 : (v < (T)0 ? (T)-1 : (T)0));
}
template <typename T> TSDE_D Dual<T> d_relu(const Dual<T>& s) {
  const T v = s.v;
  return chain(s, v > (T)0 ? v : (T)0, v > (T)0 ? (T)1 : (T)0);
}
template <typename T> TSDE_D Dual<T> d_reciprocal(const Dual<T>& s) { const T r = (T)1 / s.v; return chain(s, r, -(r * r)); }
template <typename T> TSDE_D Dual<T> d_square(const Dual<T>& s) { const T v = s.v; return chain(s, v * v, (T)2 * v); }
template <typename T> TSDE_D Dual<T> d_cube(const Dual<T>& s) { const T v = s.v; return chain(s, (v * v) * v, (T)3 * (v * v)); }
'''


def _body(words, name, dual=False):
    """Straight-line code for one program: the interpreter's stack machine (csrc/trajectory.hip ProgModel::run; `dual`:
    ProgSensModel::run) run at generation time, every instruction one `const V` statement. Returns (lines, result expression,
    constants used)."""
    lines, stack, used = [], [], set()
    count = 0
    vtype = "S" if dual else "V"

    def fresh(expr):
        nonlocal count
        var = f"{name}{count}"
        count += 1
        lines.append(f"    const {vtype} {var} = {expr};")
        return var
    for ins in words:
        op, src, k = _OPS[ins & 0xFF], (ins >> 8) & 0xFF, ins >> 16
        if (ins & 0xFF) < 16:
            if src == _SRC_STACK:
                b = stack.pop()
                a = stack.pop()
                stack.append(fresh(_BINARY[op].format(a=a, b=b)))
                continue
            if src == _SRC_CONST:
                used.add(k)
                operand = f"c{k}"
            elif src == _SRC_TIME:
                operand = f"{vtype}(time)"
            else:
                operand = "x"
            if op == "load":
                stack.append(operand)
            else:
                a = stack.pop()
                stack.append(fresh(_BINARY[op].format(a=a, b=operand)))
        elif op == "dup":
            stack.append(stack[-1])
        elif dual:
            stack.append(fresh(f"d_{op}({stack.pop()})"))
        else:
            stack.append(fresh(_UNARY[op].format(stack.pop())))
    if not stack:
        return lines, f"{vtype}((T)0)", used
    return lines, stack[-1], used


_P, _I64, _INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# family of a unit -> its one exported entry point: symbol, C parameters, their ctypes; every entry ends with _TAIL
_TAIL = ("const tsde_traj_t* tr, uint64_t entropy, uint64_t elem0, const uint64_t* entropy_dev, void* stream",
         [ctypes.POINTER(_native.Traj), ctypes.c_uint64, ctypes.c_uint64, _P, _P])
_ENTRY = {
    "values": ("tsde_specialised_launch",
               "void* ys, const void* y0, int64_t rows, int64_t d, const void* consts, int n_const, int scalar_noise",
               [_P, _P, _I64, _I64, _P, _INT, _INT]),
    "sens": ("tsde_specialised_sens_launch",
             "void* ys, void* sens, const int8_t* param_slot, const void* y0, int64_t rows, int64_t d, const void* consts, "
             "int n_const, int scalar_noise", [_P, _P, _P, _P, _I64, _I64, _P, _INT, _INT]),
    "additive": ("tsde_specialised_additive_launch",
                 "void* ys, const void* y0, int64_t rows, int64_t d, int64_t m, const void* consts, int n_const, "
                 "const void* gtab, int time_dependent", [_P, _P, _I64, _I64, _I64, _P, _INT, _P, _INT]),
    "rows": ("tsde_specialised_rows_launch", "void* ys, const void* y0, int64_t rows, int64_t d, const void* consts, int n_const",
             [_P, _P, _I64, _I64, _P, _INT]),
    "rows_sens": ("tsde_specialised_rows_sens_launch",
                  "void* ys, void* sens, const void* y0, int64_t rows, int64_t d, const void* consts, int n_const",
                  [_P, _P, _P, _I64, _I64, _P, _INT]),
    "rows_general": ("tsde_specialised_rows_general_launch",
                     "void* ys, const void* y0, int64_t rows, int64_t d, const void* consts, int n_const, int64_t m",
                     [_P, _P, _I64, _I64, _P, _INT, _I64]),
}


def _family(kind):
    return kind.rstrip("0123456789")          # ("additive8": the additive family, channel-count class 8)


def _unit(note, model, kind, dtype, method, refuse, scalar_noise, call):
    """A translation unit: the kernels' source, the generated model, and the entry point of `kind` -- which refuses arguments
    the model was not generated for (`refuse`) and hands everything else to the launch helpers of csrc/trajectory.hip."""
    symbol, params, _ = _ENTRY[_family(kind)]
    return f'''// generated by torchsde_amd/specialise.py{note} -- do not edit
#define TSDE_SPECIALISE_TU 1
#include "{os.path.join(_CSRC, "trajectory.hip")}"
namespace tsde {{
{model}}}  // namespace tsde

extern "C" int {symbol}({params}, {_TAIL[0]}) {{
  using namespace tsde;
  using T = {"float" if dtype == torch.float32 else "double"};
  constexpr int METHOD = {int(method)};
  if ({refuse}) return (int)hipErrorInvalidValue;
  const hipStream_t s = (hipStream_t)stream;
  const ProgArgs<T> p = prog_args<T>(ys, y0, rows, d, consts, n_const, {scalar_noise}, tr, noise_key(entropy, elem0), entropy_dev);
  return (int){call};
}}
'''


def _model(struct, value, members, setup, bodies, v2):
    """A generated model, with the interface of the interpreter's (csrc/trajectory.hip ProgModel, ProgSensModel). `struct`: its
    template head and name; `value`: the alias of its value type (V, or S on dual numbers); `members`, `setup`: its constants
    and how a lane loads them; `bodies`: of eval_f, eval_g and, where the derivative schemes run, eval_h; `v2`: the type of gdg's
    last argument."""
    V = value.split()[0]
    evals = "".join(f"  TSDE_D {V} eval_{name}(const {V}& x, const T time) const {{\n{body}\n  }}\n" for name, body in bodies.items())
    gdg = "(gv * v2) * eval_h(x, tslot[SLOT])" if "h" in bodies else f"{V}((T)0)"
    return f'''{struct} {{
  using {value};
{members}  T tslot[4];
{setup}{evals}  template <int SLOT>
  TSDE_D {V} f(const {V}& x) const {{ return eval_f(x, tslot[SLOT]); }}
  template <int SLOT>
  TSDE_D {V} g(const {V}& x) const {{ return eval_g(x, tslot[SLOT]); }}
  template <int SLOT>
  TSDE_D {V} gdg(const {V}& x, const {V}& gv, {v2} v2) const {{ return {gdg}; }}
}};
'''


def source(f_code, g_code, dg_code, n_const, dtype, method, kind="values"):
    """The translation unit for these programs, this state dtype and this scheme. `kind`: "values"
    (`trajectory_prog_kernel`), "sens" (`trajectory_prog_sens_kernel`: the programs on dual numbers), or "additive<MP>"
    (`trajectory_prog_additive_kernel` for ONE channel-count class, the drift program alone)."""
    dual = kind == "sens"
    bodies, used = {}, set()
    for name, words in (("f", f_code), ("g", g_code), ("h", dg_code)):
        lines, result, consts = _body(tuple(words), name, dual)
        bodies[name] = "\n".join(lines + [f"    return {result};"])
        used |= consts
    used = sorted(used)
    short = f"n_const < {(used[-1] + 1) if used else 0}"
    if dual:
        setup = "".join(f"    c{k} = S(q.base.consts[(int64_t){k} * q.base.d + column]);\n"
                        f"    if (q.param_slot[{k}] > 0) c{k}.d[q.param_slot[{k}]] = (T)1;\n" for k in used)
        model = _DUAL_HELPERS + _model("template <typename T>\nstruct SpecSensModel", "S = Dual<T>",
                                       "".join(f"  S c{k};\n" for k in used),
                                       f"  TSDE_D void setup(const ProgSensArgs<T>& q, int64_t column) {{\n{setup}  }}\n", bodies, "T")
        return _unit("", model, kind, dtype, method, f"{short} || n_const > kProgParamRows", "scalar_noise",
                     "launch_prog_sens_m<T, METHOD, SpecSensModel<T>>(prog_sens_args(p, sens, param_slot), s)")
    setup = "".join(f"    {{ const Pack<T, W> pk = load<T, W>(p.consts, (int64_t){k} * p.d + column);\n"
                    f"      _Pragma(\"unroll\") for (int q = 0; q < W; ++q) c{k}.v[q] = pk.v[q]; }}\n" for k in used)
    model = _model("template <typename T, int W>\nstruct SpecModel", "V = Vec<T, W>", "".join(f"  V c{k};\n" for k in used),
                   f"  TSDE_D void setup(const ProgArgs<T>& p, int64_t column) {{\n{setup}  }}\n", bodies, "const V&")
    if kind == "values":
        return _unit("", model, kind, dtype, method, short, "scalar_noise", "launch_prog_m<T, METHOD, SpecModel>(p, s)")
    mp = int(kind[len("additive"):])
    return _unit("", model, kind, dtype, method, f"{short} || m < 1 || m > {mp}", "0",
                 f"launch_additive_mp<T, METHOD, {mp}, SpecModel>(prog_additive_args(p, m, gtab, time_dependent, METHOD), s)")


# ---- compiling, caching, loading -------------------------------------------------------------------------------------------
_lock = threading.Lock()
_state = {}            # key -> "pending" | "failed: ..." | _Library
_verified = {}         # key -> True | False (the specialised launch reproduced the interpreter bit for bit)


class _Library:
    def __init__(self, path, kind):
        self.path = path
        self.lib = ctypes.CDLL(path)
        symbol, _, argtypes = _ENTRY[_family(kind)]
        self.launch = getattr(self.lib, symbol)
        self.launch.argtypes = argtypes + _TAIL[1]
        self.launch.restype = ctypes.c_int


def cache_dir():
    """Where the compiled units live: ``TSDE_SPECIALISE_CACHE``, else under ``~/.cache``; a home that cannot be written to
    (a container's read-only user) falls back to the system's temporary directory."""
    import tempfile
    wanted = os.environ.get("TSDE_SPECIALISE_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "torchsde_amd", "specialised")
    for root in (wanted, os.path.join(tempfile.gettempdir(), f"torchsde_amd_specialised_{os.getuid()}")):
        try:
            os.makedirs(root, exist_ok=True)
            if os.access(root, os.W_OK):
                return root
        except OSError:
            continue
    raise OSError(f"no writable directory for compiled programs (tried {wanted} and the temporary directory)")


def compiler():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
                                                               else None)


def _arch(device):
    try:
        return torch.cuda.get_device_properties(device).gcnArchName.split(":")[0]
    except Exception:
        return "gfx950"


def _compile_command(arch, out, src):
    return [compiler(), "-O3", "-std=c++17", "-fPIC", f"--offload-arch={arch}", "-ffp-contract=off", "-shared", "-o", out, src]


def _compile(key, text, arch, kind="values"):
    try:
        path = os.path.join(cache_dir(), f"{key}.so")
        if not os.path.exists(path):
            src = os.path.join(cache_dir(), f"{key}.hip")
            with open(src, "w") as fh:
                fh.write(text)
            tmp = f"{path}.{os.getpid()}.{threading.get_ident()}.tmp"
            done = subprocess.run(_compile_command(arch, tmp, src), capture_output=True, text=True, timeout=600)
            if done.returncode != 0:
                raise RuntimeError(done.stderr[-2000:])
            os.replace(tmp, path)                 # (atomic: another process may be compiling the same key)
        result = _Library(path, kind)
    except Exception as e:       # no compiler, a compile error, a load error: the interpreter stays
        result = f"failed: {type(e).__name__}: {e}"
    with _lock:
        _state[key] = result


def _find(make_text, kind, device, wait):
    """(key, the loaded library of the unit `make_text()` or None). The first call starts the compilation (in the background
    unless TSDE_SPECIALISE=sync or `wait`)."""
    if MODE in ("0", "false", "off") or compiler() is None:
        return None, None
    arch = _arch(device)
    text = make_text()
    key = hashlib.sha256((text + arch + _sources_digest()).encode()).hexdigest()[:24]
    with _lock:
        have = _state.get(key)
        if have is None:
            _state[key] = "pending"
    if have is None:
        if MODE == "sync" or wait:
            _compile(key, text, arch, kind)
        elif not _enqueue(key, text, arch, kind):
            with _lock:
                _state.pop(key, None)            # (the queue is full: ask again at a later solve)
        with _lock:
            have = _state.get(key)
    return key, (have if isinstance(have, _Library) else None)


def lookup(f_code, g_code, dg_code, n_const, dtype, method, device, wait=None, kind="values"):
    """(key, library or None) of these programs (`_find`)."""
    return _find(lambda: source(f_code, g_code, dg_code, n_const, dtype, method, kind), kind, device, wait)


# one worker, a short queue: a process that meets hundreds of different programs (a test-suite) compiles a few at a time
_queue = None


def _enqueue(*job):
    global _queue
    import queue
    with _lock:
        if _queue is None:
            _queue = queue.Queue(maxsize=8)

            def work():
                while True:
                    _compile(*_queue.get())
            threading.Thread(target=work, daemon=True, name="torchsde_amd-specialise").start()
    try:
        _queue.put_nowait(job)
        return True
    except queue.Full:
        return False


_digest = None


def _sources_digest():
    """Hash of the kernel sources a specialised unit includes: a changed header must not find a stale cached library."""
    global _digest
    if _digest is None:
        h = hashlib.sha256()
        for name in sorted(os.listdir(_CSRC)):
            if name.endswith((".h", ".hip")):
                with open(os.path.join(_CSRC, name), "rb") as fh:
                    h.update(fh.read())
        with open(os.path.join(os.path.dirname(_HERE), "include", "torchsde_amd.h"), "rb") as fh:
            h.update(fh.read())
        _digest = h.hexdigest()
    return _digest


def status():
    """{key: "pending" | "failed: ..." | path} of every program seen by this process (diagnostics)."""
    with _lock:
        return {k: (v.path if isinstance(v, _Library) else v) for k, v in _state.items()}


def verified(key):
    return _verified.get(key)


def set_verified(key, ok):
    _verified[key] = bool(ok)


def launch(library, schedule, bm, stream, *args):
    """One launch of a compiled unit: `args` are its entry point's own arguments (`_ENTRY`), the schedule, the noise key and the
    stream follow."""
    lib = _native.load()
    slot = lib.tsde_prof_bracket_open(_native.KID_TRAJECTORY, stream)       # (bench.py's per-launch timing of this kernel family)
    rc = library.launch(*args, *_native.trajectory_tail(schedule, bm, stream))
    if slot >= 0:
        lib.tsde_prof_bracket_close(slot, stream)
    if rc != 0:
        raise _native.NativeLibraryError(f"torchsde_amd: a specialised program kernel failed with hipError {rc}")


# ---- row-coupled systems: a lane owns a whole row (recognise_rows.py) --------------------------------------------------------
_ROW_OPS = {
    "add": "({0} + {1})", "sub": "({0} - {1})", "mul": "({0} * {1})", "div": "({0} / {1})", "neg": "(-{0})",
    "exp": "exp({0})", "log": "log({0})", "sin": "sin({0})", "cos": "cos({0})", "tanh": "tanh({0})",
    "sigmoid": "((T)1 / ((T)1 + exp(-{0})))", "softplus": "({0} > (T)20 ? {0} : log1p(exp({0})))", "sqrt": "sqrt({0})",
    "abs": "fabs({0})", "relu": "({0} > (T)0 ? {0} : (T)0)", "reciprocal": "((T)1 / {0})", "square": "({0} * {0})",
    "cube": "(({0} * {0}) * {0})",
}


def source_rows(structure, n_const, dtype, method):
    """The translation unit of a row-coupled system: `structure` = RecognisedRows.structure(). (No derivative schemes on this
    route: the model has no eval_h.)"""
    (_, d, statements, outputs), _ = structure
    names = [f"n{k}" for k in range(len(statements))]
    needs = {}
    for name, (op, operands) in zip(names, statements):
        needs[name] = set(o for o in operands if o in needs or o.startswith("n"))

    def body(outs):
        wanted, stack = set(), [o for o in outs if o.startswith("n")]
        while stack:
            x = stack.pop()
            if x in wanted:
                continue
            wanted.add(x)
            stack.extend(o for o in needs.get(x, ()) if o.startswith("n"))
        lines = [f"    const T {name} = {_ROW_OPS[op].format(*operands)};" for name, (op, operands) in zip(names, statements)
                 if name in wanted]
        lines.append("    V r;")
        lines += [f"    r.v[{c}] = {o};" for c, o in enumerate(outs)]
        lines.append("    return r;")
        return "\n".join(lines)
    nc = max(1, n_const)
    setup = f"""  TSDE_D void setup(const ProgArgs<T>& p, int64_t) {{
    _Pragma("unroll") for (int k = 0; k < {nc}; ++k) c[k] = k < p.n_const ? p.consts[k] : (T)0;
  }}
"""
    model = _model("template <typename T>\nstruct RowModel", f"V = Vec<T, {d}>", f"  T c[{nc}];\n", setup,
                   {"f": body(list(outputs[:d])), "g": body(list(outputs[d:]))}, "const V&")
    return _unit(" (a row-coupled system)", model, "rows", dtype, method, f"d != {d} || n_const > {nc}", "0",
                 f"launch_prog_w<T, METHOD, {d}, RowModel<T>>(p, s)")


def lookup_rows(structure, n_const, dtype, method, device, wait=None):
    """(key, library or None) of a row-coupled system (`_find`)."""
    return _find(lambda: source_rows(structure, n_const, dtype, method), "rows", device, wait)


# ---- ... and their path-wise sensitivities (csrc/trajectory.hip trajectory_rows_sens_kernel) ----------------------------------
def rows_sens_tangents(d, slots, y0_grad):
    """NT of a tangent unit: the row's d slots for y0 (if it needs a gradient), then one per trainable scalar."""
    return (d if y0_grad else 0) + (max(slots) + 1 if slots and max(slots) >= 0 else 0)


def _row_tangent_helpers():
    """The slope rules of the elementwise programs (`_DUAL_HELPERS`, ProgSensModel::run) for `Tan<T, NT>`: the one table,
    retyped."""
    return _DUAL_HELPERS.replace("template <typename T>", "template <typename T, int NT>").replace("Dual<T>", "Tan<T, NT>")


def source_rows_sens(structure, n_const, dtype, method, slots, y0_grad):
    """The translation unit of a row-coupled system WITH tangents: the statements of `source_rows` in the same order, each
    scalar node a value plus NT tangents (`Tan<T, NT>`) wherever the state or a trainable constant reaches it -- nodes they do
    not reach stay plain `T`, statement for statement what `source_rows` emits. `slots[k]`: the tangent slot of constant k among
    the trainable scalars, or -1; `y0_grad`: the state's channels carry the first d slots. The value part of every dual
    operation is the plain statement's expression (trajectory.hip `Tan`, `_DUAL_HELPERS`), hence the same `ys`."""
    (_, d, statements, outputs), _ = structure
    slots = tuple(int(s) for s in slots)
    d0 = d if y0_grad else 0
    nt = rows_sens_tangents(d, slots, y0_grad)
    if nt < 1:
        raise ValueError("a tangent unit needs a gradient to carry")
    names = [f"n{k}" for k in range(len(statements))]
    needs = {name: set(o for o in operands if o.startswith("n")) for name, (op, operands) in zip(names, statements)}
    dual = {}                    # statement name -> whether it carries tangents

    def is_dual(o):
        if o.startswith("x.v["):
            return True
        if o.startswith("c["):
            k = int(o[2:-1])
            return k < len(slots) and slots[k] >= 0
        return dual.get(o, False)

    def spell(o):
        if o.startswith("x.v["):
            return f"x{int(o[4:-1])}"
        if o.startswith("c[") and is_dual(o):
            return f"k{int(o[2:-1])}"
        return o
    for name, (op, operands) in zip(names, statements):
        dual[name] = any(is_dual(o) for o in operands)

    def body(outs):
        wanted, stack = set(), [o for o in outs if o.startswith("n")]
        while stack:
            x = stack.pop()
            if x in wanted:
                continue
            wanted.add(x)
            stack.extend(needs.get(x, ()))
        used = [(name, op, operands) for name, (op, operands) in zip(names, statements) if name in wanted]
        leaves = [o for _, _, operands in used for o in operands] + list(outs)
        lines = [f"    const N x{c} = x.channel({c});" for c in range(d) if f"x.v[{c}]" in leaves]
        lines += [f"    const N k{k} = tan_seed<{d0 + slots[k]}, T, {nt}>(c[{k}]);" for k in range(len(slots))
                  if slots[k] >= 0 and f"c[{k}]" in leaves]
        for name, op, operands in used:
            if not dual[name]:
                lines.append(f"    const T {name} = {_ROW_OPS[op].format(*operands)};")
            elif len(operands) == 1:
                lines.append(f"    const N {name} = d_{op}({spell(operands[0])});")
            else:
                lines.append(f"    const N {name} = {_ROW_OPS[op].format(*[spell(o) for o in operands])};")
        lines.append("    S r;")
        lines += [f"    r.set({c}, {spell(o)});" for c, o in enumerate(outs)]
        lines.append("    return r;")
        return "\n".join(lines)
    nc = max(1, n_const)
    setup = f"""  static constexpr bool kStateSlots = {"true" if y0_grad else "false"};
  TSDE_D void setup(const ProgArgs<T>& p, int64_t) {{
    _Pragma("unroll") for (int k = 0; k < {nc}; ++k) c[k] = k < p.n_const ? p.consts[k] : (T)0;
  }}
"""
    model = _row_tangent_helpers() + _model("template <typename T>\nstruct RowSensModel", f"S = RowTan<T, {d}, {nt}>",
                                            f"  using N = Tan<T, {nt}>;\n  T c[{nc}];\n", setup,
                                            {"f": body(list(outputs[:d])), "g": body(list(outputs[d:]))}, "const Vec<T, " + str(d) + ">&")
    return _unit(f" (a row-coupled system with {nt} tangents)", model, "rows_sens", dtype, method,
                 f"d != {d} || n_const > {nc} || sens == nullptr", "0",
                 f"launch_rows_sens<T, METHOD, {d}, {nt}, RowSensModel<T>>(p, sens, s)")


def lookup_rows_sens(structure, n_const, dtype, method, slots, y0_grad, device, wait=None):
    """(key, library or None) of a row-coupled system's tangent unit (`_find`)."""
    return _find(lambda: source_rows_sens(structure, n_const, dtype, method, slots, y0_grad), "rows_sens", device, wait)


# Which systems take the tangent unit. A lane keeps d * (NT + 1) numbers per state and a scheme keeps several states alive
# (SRK: the stages' drifts and diffusions); past a size the compiler spills them and the launch loses to the stepwise route.
# Per scheme and dtype, a cap on d * (NT + 1) that lies below the first worst-case unit OF ANY d = 2 .. 8 -- a dense synthetic
# system, every drift and diffusion channel reading every state channel and a trainable constant -- that compiles for gfx950
# with scratch or spilled vector registers (tools/rows_sens_resource_usage.py, profiles/rows_sens_resource_usage.txt: every
# admitted (d, NT) is listed there and fits); NT <= 16 throughout. float64 takes two registers per number. The narrow rows set
# several float32 caps: the register allocator does worse at d = 5 and 7 than at 8 (SRK spills at 5 x 3 and not at 6 x 4).
ROWS_SENS_MAX_TANGENTS = 16
ROWS_SENS_CAP = {      # method code -> cap on d * (NT + 1) in (float32, float64)
    _native.TRAJ_EULER: (84, 32), _native.TRAJ_MIDPOINT: (69, 32), _native.TRAJ_HEUN: (56, 16),
    _native.TRAJ_EULER_HEUN: (55, 24), _native.TRAJ_SRK: (14, 16),
}


def rows_sens_refusal(d, nt, method, dtype):
    """Why a system of d channels with nt tangents stays stepwise under this scheme, or None."""
    cap = ROWS_SENS_CAP.get(int(method))
    if cap is None:
        return "no tangent kernel for this scheme"
    cap = cap[0 if dtype == torch.float32 else 1]
    if nt > ROWS_SENS_MAX_TANGENTS:
        return f"{nt} tangents per row (y0's channels and the trainable scalars), more than {ROWS_SENS_MAX_TANGENTS}"
    if d * (nt + 1) > cap:
        return (f"{d} channels x ({nt} tangents + 1) = {d * (nt + 1)} numbers per state, more than the {cap} this scheme keeps "
                "in registers")
    return None


# ---- ... and row-coupled systems with a diffusion MATRIX (csrc/trajectory.hip trajectory_rows_general_kernel) ------------------
def source_rows_general(structure, n_const, dtype, method):
    """The translation unit of a row-coupled system with general, scalar or additive noise: `structure` =
    RecognisedRows.structure() of `recognise_rows(..., m=m)`, outputs = d drift expressions, then the d * m entries of the
    diffusion matrix row-major. The model is `source_rows`' statements plus a GENERATED CONTRACTION with the step's increments
    `w` (the kernel writes them into the model before every step): per row i, `sum_k g_ik * w[k]` in increasing k, straight-line,
    with no term for an entry that is the literal 0 -- the matrix never exists as an array, Heston costs three products per
    stage. `g<SLOT>(x)` returns that vector, so `scheme_step` runs the schemes with the unit as their noise operand."""
    (_, d, m, statements, outputs), _ = structure
    names = [f"n{k}" for k in range(len(statements))]
    needs = {name: set(o for o in operands if o.startswith("n")) for name, (op, operands) in zip(names, statements)}

    def structural_zero(o):
        return o.startswith("(T)") and float(o[3:]) == 0.0

    def lines_for(outs):
        wanted, stack = set(), [o for o in outs if o.startswith("n")]
        while stack:
            x = stack.pop()
            if x in wanted:
                continue
            wanted.add(x)
            stack.extend(needs.get(x, ()))
        return [f"    const T {name} = {_ROW_OPS[op].format(*operands)};" for name, (op, operands) in zip(names, statements)
                if name in wanted]
    drift = list(outputs[:d])
    f_body = lines_for(drift) + ["    V r;"] + [f"    r.v[{c}] = {o};" for c, o in enumerate(drift)] + ["    return r;"]
    entries = list(outputs[d:])
    live = [o for o in entries if not structural_zero(o)]
    g_body = lines_for(live) + ["    V r;"]
    for i in range(d):
        total = None
        for k in range(m):
            o = entries[i * m + k]
            if structural_zero(o):
                continue
            term = f"{o} * w[{k}]"
            total = term if total is None else f"({total}) + {term}"
        g_body.append(f"    r.v[{i}] = {total if total is not None else '(T)0'};")
    g_body.append("    return r;")
    nc = max(1, n_const)
    setup = f"""  TSDE_D void setup(const ProgArgs<T>& p, int64_t) {{
    _Pragma("unroll") for (int k = 0; k < {nc}; ++k) c[k] = k < p.n_const ? p.consts[k] : (T)0;
  }}
"""
    model = _model("template <typename T>\nstruct RowGeneralModel", f"V = Vec<T, {d}>", f"  T c[{nc}];\n  T w[{m}];\n", setup,
                   {"f": "\n".join(f_body), "g": "\n".join(g_body)}, "const T&")
    return _unit(f" (a row-coupled system, {m} Brownian channels)", model, "rows_general", dtype, method,
                 f"d != {d} || m != {m} || n_const > {nc}", "0",
                 f"launch_rows_general<T, METHOD, {d}, {m}, RowGeneralModel<T>>(p, m, s)")


def lookup_rows_general(structure, n_const, dtype, method, device, wait=None):
    """(key, library or None) of a row-coupled system with a diffusion matrix (`_find`)."""
    return _find(lambda: source_rows_general(structure, n_const, dtype, method), "rows_general", device, wait)


# Which (d, m) take that unit. A lane keeps the row's d values, the m increments and, per stage, d drift values and the d sums of
# the contraction; the entries of the matrix are consumed as they are made. Per scheme and dtype a cap on d * m that lies below
# the first (d, m), d = 1 .. 8, m = 1 .. 8, whose DENSE worst case (tests/helpers_rows_general.DenseWorst: every entry reads
# every channel, a constant of its own and t) compiles for gfx950 with scratch or spilled vector registers
# (tools/rows_general_resource_usage.py, profiles/rows_general_resource_usage.txt: every pair is listed there).
ROWS_GENERAL_CAP = {   # method code -> cap on d * m in (float32, float64)
    _native.TRAJ_EULER: (64, 64), _native.TRAJ_MIDPOINT: (64, 64), _native.TRAJ_HEUN: (64, 64),
    _native.TRAJ_EULER_HEUN: (64, 64),
}


def rows_general_refusal(d, m, method, dtype):
    """Why a system of d channels and m Brownian channels stays stepwise under this scheme, or None."""
    cap = ROWS_GENERAL_CAP.get(int(method))
    if cap is None:
        return "no row kernel with a diffusion matrix for this scheme"
    cap = cap[0 if dtype == torch.float32 else 1]
    if d * m > cap:
        return f"{d} channels x {m} Brownian channels = {d * m} matrix entries, more than the {cap} this scheme keeps in registers"
    return None
