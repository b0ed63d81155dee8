"""ctypes binding of libg4d_hip.so (the C ABI declared in include/g4d.h).

The library is built in-tree (garment4d_amd/lib/libg4d_hip.so) by `__graft_entry__.build()` /
`make -C garment4d_amd/csrc`.  There is NO fallback: if the library is missing, or a call fails,
this raises -- the product path never silently routes to PyTorch eager or to the CPU oracle.

Nothing of the ABI is typed here by hand: every prototype's argtypes and restype, the fields of `g4d_mlp_args` and the `G4D_*` constants
are read from include/g4d.h when the library is loaded (`parse_header`), and tests/abi_snapshot.txt is the reviewed record of what that
gives -- a changed or new entry point shows up there as a changed or new line.

Further libraries of the package are (header, library) pairs of the same shape, loaded by load_pair(): the rasterizer, include/g4d_render.h +
lib/libg4d_render.so (render_lib(); record: tests/render_abi_snapshot.txt), and the virtual depth-sensor scans, include/g4d_scan.h +
lib/libg4d_scan.so (scan_lib(); record: tests/scan_abi_snapshot.txt), and the point-to-surface loss, include/g4d_fit.h + lib/libg4d_fit.so
(fit_lib(); record: tests/fit_abi_snapshot.txt), and the adjoint of lbs(), include/g4d_smpl.h + lib/libg4d_smpl.so (smpl_lib(); record:
tests/smpl_abi_snapshot.txt), and the adjoint of the garment skinning, include/g4d_skin.h + lib/libg4d_skin.so (skin_lib(); record:
tests/skin_abi_snapshot.txt), and the projective ray-depth loss, include/g4d_depth.h + lib/libg4d_depth.so (depth_lib(); record:
tests/depth_abi_snapshot.txt).  call() serves them too.  include/g4d_sets.h is a further header of
libg4d_hip.so ITSELF (sets_lib(); record: tests/sets_abi_snapshot.txt): entry points added after g4d.h's record was closed; include/g4d_live.h
is another (live_lib(); record: tests/live_abi_snapshot.txt): the live-cloud scope, opened from Python with live_scope().
"""
import contextlib
import ctypes
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("G4D_LIB_PATH") or os.path.join(_HERE, "lib", "libg4d_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d.h")

# the second (header, library) pair: the rasterizer (include/g4d_render.h, libg4d_render.so; render_lib() loads it).  It links against
# libg4d_hip.so and reports through the same g4d_last_error().  The names PROTOTYPES, SIGNATURES, RESTYPES, _lib, _header stay g4d.h's alone.
RENDER_LIB_PATH = os.path.join(_HERE, "lib", "libg4d_render.so")
RENDER_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_render.h")
# the third pair, of the same shape: virtual depth-sensor scans (include/g4d_scan.h, libg4d_scan.so; scan_lib() loads it)
SCAN_LIB_PATH = os.path.join(_HERE, "lib", "libg4d_scan.so")
SCAN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_scan.h")
# the fourth pair: point-to-surface loss and its gradient (include/g4d_fit.h, libg4d_fit.so; fit_lib() loads it)
FIT_LIB_PATH = os.path.join(_HERE, "lib", "libg4d_fit.so")
FIT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_fit.h")
# the fifth pair: the adjoint of lbs() (include/g4d_smpl.h, libg4d_smpl.so; smpl_lib() loads it)
SMPL_LIB_PATH = os.path.join(_HERE, "lib", "libg4d_smpl.so")
SMPL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_smpl.h")
# the sixth pair: the adjoint of the garment skinning (include/g4d_skin.h, libg4d_skin.so; skin_lib() loads it)
SKIN_LIB_PATH = os.path.join(_HERE, "lib", "libg4d_skin.so")
SKIN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_skin.h")
# the seventh pair: the projective ray-depth loss and its gradient (include/g4d_depth.h, libg4d_depth.so; depth_lib() loads it)
DEPTH_LIB_PATH = os.path.join(_HERE, "lib", "libg4d_depth.so")
DEPTH_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_depth.h")

# a further header of libg4d_hip.so itself (no library of its own): entry points that came after the record of g4d.h (sets_lib() binds them)
SETS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_sets.h")
# ... and the live-cloud scope of the same library (live_lib() binds it, live_scope() opens one)
LIVE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g4d_live.h")

_lib = None
_header = None   # HEADER_PATH once the names below are bound from it
_more = {}       # (header path, library path) -> (its CDLL, {entry point: (restype, argtypes)}, its G4D_* constants) of every further pair load_pair() loaded


class G4DError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint}


def _ctype(decl, where, named=True):
    """The ctypes type of one C declaration of include/g4d.h (`const float *const *scale`, `long long rows`, a return type with
    named=False): any pointer and g4d_stream_t -> c_void_p, `const char *` -> c_char_p, the scalars of _SCALARS; anything else raises."""
    base, star, rest = decl.partition("*")
    words = [w for w in base.split() if w != "const"]
    if named and not star:
        words.pop()   # the parameter's / field's own name
    base = " ".join(words)
    if star:
        return ctypes.c_char_p if base == "char" and "*" not in rest else ctypes.c_void_p
    if base == "g4d_stream_t":
        return ctypes.c_void_p
    if base not in _SCALARS:
        raise G4DError(f"include/g4d.h: {where}: no ctypes type known for `{' '.join(decl.split())}`")
    return _SCALARS[base]


def parse_header(text):
    """include/g4d.h -> ({entry point: (restype, [argtypes])}, [(field, type)] of g4d_mlp_args, {G4D_* #define or enumerator: int}).
    Reads that header and nothing else: comments and preprocessor lines are dropped, the rest is cut into statements at ; { }."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(G4D_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for body in re.findall(r"\benum\s+\w+\s*\{(.*?)\}", text, flags=re.S):
        consts.update((n, int(v, 0)) for n, v in re.findall(r"(G4D_\w+)\s*=\s*(-?\w+)", body))
    fields = []
    struct = re.search(r"\bstruct\s+g4d_mlp_args\s*\{(.*?)\}", text, flags=re.S)
    for decl in filter(str.strip, struct.group(1).split(";") if struct else ()):
        first, *more = decl.split(",")
        base = first.partition("*")[0] if "*" in first else first.rsplit(None, 1)[0]   # `const float *a, *const *b, c`: the type without the first name
        for piece in [first] + [base + " " + p for p in more]:
            fields.append((re.findall(r"\w+", piece)[-1], _ctype(piece, "g4d_mlp_args")))
    protos = {}
    for stmt in re.split(r"[;{}]", text):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(g4d_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            raise G4DError(f"include/g4d.h: cannot read `{' '.join(stmt.split())}` as a prototype")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("void", "") else params.split(",")
        protos[name] = (_ctype(ret, name, named=False), [_ctype(p, name) for p in params])
    return protos, fields, consts


# what call() shows a g4d_mlp_run as in traces and timing tables: the positional entry point of the family, keyed by the header's enumerator
_MLP_FAMILY_LABELS = {"G4D_MLP_STACK_F32": "g4d_mlp_stack_f32", "G4D_MLP_STACK_BF16": "g4d_mlp_stack_bf16", "G4D_MLP_WAVE_F32": "g4d_mlp_wave_f32",
                      "G4D_MLP_CHAIN_F32": "g4d_mlp_chain_f32", "G4D_MLP_CHAIN_BF16": "g4d_mlp_chain_bf16", "G4D_MLP_CHAIN_BF16X3": "g4d_mlp_chain_bf16x3"}


def _bind_header():
    """Read include/g4d.h and define the module's derived names from it: PROTOTYPES (name -> (restype, argtypes)), SIGNATURES (name ->
    argtypes), RESTYPES (name -> restype where it is not c_int), CONSTANTS (every integer G4D_* #define and enumerator), MLP_ARGS_VERSION,
    MLP_STACK_F32 ... MLP_CHAIN_BF16X3 (enum g4d_mlp_family) and MlpArgs."""
    global _header
    try:
        with open(HEADER_PATH) as f:
            protos, fields, consts = parse_header(f.read())
    except OSError as e:
        raise G4DError(f"{HEADER_PATH} cannot be read ({e.strerror}): the ctypes binding is derived from it. There is no fallback table.")

    class MlpArgs(ctypes.Structure):
        """include/g4d.h `g4d_mlp_args`, read from the header -- the ONE argument block of the whole-stack launchers (g4d_mlp_run).
        tests/test_abi_cpu.py checks sizeof against the library's g4d_mlp_args_size() and the fields against tests/abi_snapshot.txt."""
        _fields_ = fields

        def __init__(self, **kw):
            super().__init__(size=ctypes.sizeof(MlpArgs), version=consts["G4D_MLP_ARGS_VERSION"], tap_layer=-1, **kw)

    globals().update(
        PROTOTYPES=protos, SIGNATURES={n: a for n, (r, a) in protos.items()}, RESTYPES={n: r for n, (r, a) in protos.items() if r is not ctypes.c_int},
        CONSTANTS=consts, MlpArgs=MlpArgs, _MLP_FAMILY_NAMES={consts[k]: v for k, v in _MLP_FAMILY_LABELS.items()},
        **{k[4:]: v for k, v in consts.items() if k.startswith("G4D_MLP_")})   # MLP_ARGS_VERSION and the families
    _header = HEADER_PATH


def __getattr__(name):
    # the derived names, for code that reads them before lib() has loaded the library (numerics.MODES, tests of the tables)
    if _header is None and not name.startswith("__"):
        _bind_header()
        if name in globals():
            return globals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def lib():
    """Load libg4d_hip.so once, typed as include/g4d.h declares it; raise (loudly) when either is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise G4DError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import "
                f"__graft_entry__ as g; g.build()'` (or `make -C garment4d_amd/csrc`). There is no fallback path.")
        if _header is None:
            _bind_header()
        # torch first: its wheel bundles a libamdhip64; loading ours before it would bring in /opt/rocm's copy as a SECOND HIP runtime
        # in the process, and the library's launches would then run in a runtime that never saw torch's device / streams
        # ("no ROCm-capable device is detected" from the first hipFuncSetAttribute)
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def load_pair(header_path, lib_path):
    """Load a further library once, typed as its own header declares it (the same parse as include/g4d.h's): call() then finds its entry
    points.  libg4d_hip.so is loaded first -- such a library links against it and shares its error state.  Returns (CDLL, prototypes, constants)."""
    key = (header_path, lib_path)   # (libg4d_hip.so itself is the library of more than one further header)
    if key not in _more:
        lib()
        if not os.path.exists(lib_path):
            raise G4DError(f"{lib_path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"(or `make -C garment4d_amd/csrc`). There is no fallback path.")
        try:
            with open(header_path) as f:
                protos, _, consts = parse_header(f.read())
        except OSError as e:
            raise G4DError(f"{header_path} cannot be read ({e.strerror}): the ctypes binding is derived from it. There is no fallback table.")
        L = ctypes.CDLL(lib_path)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.argtypes = argtypes
            fn.restype = restype
        _more[key] = (L, protos, consts)
    return _more[key]


def render_lib():
    """libg4d_render.so typed from include/g4d_render.h: (CDLL, prototypes, constants)."""
    return load_pair(RENDER_HEADER_PATH, RENDER_LIB_PATH)


def scan_lib():
    """libg4d_scan.so typed from include/g4d_scan.h: (CDLL, prototypes, constants)."""
    return load_pair(SCAN_HEADER_PATH, SCAN_LIB_PATH)


def fit_lib():
    """libg4d_fit.so typed from include/g4d_fit.h: (CDLL, prototypes, constants)."""
    return load_pair(FIT_HEADER_PATH, FIT_LIB_PATH)


def smpl_lib():
    """libg4d_smpl.so typed from include/g4d_smpl.h: (CDLL, prototypes, constants)."""
    return load_pair(SMPL_HEADER_PATH, SMPL_LIB_PATH)


def skin_lib():
    """libg4d_skin.so typed from include/g4d_skin.h: (CDLL, prototypes, constants)."""
    return load_pair(SKIN_HEADER_PATH, SKIN_LIB_PATH)


def depth_lib():
    """libg4d_depth.so typed from include/g4d_depth.h: (CDLL, prototypes, constants)."""
    return load_pair(DEPTH_HEADER_PATH, DEPTH_LIB_PATH)


def sets_lib():
    """libg4d_hip.so's entry points of include/g4d_sets.h, typed from that header: (CDLL, prototypes, constants)."""
    return load_pair(SETS_HEADER_PATH, LIB_PATH)


def live_lib():
    """libg4d_hip.so's entry points of include/g4d_live.h, typed from that header: (CDLL, prototypes, constants)."""
    return load_pair(LIVE_HEADER_PATH, LIB_PATH)


@contextlib.contextmanager
def live_scope(count, capacity):
    """Launches made (or captured) by this thread inside the block honour a live-cloud count read on the device (include/g4d_live.h): `count`
    is a one-element int32 HIP tensor -- kept alive, and rewritten on the launching stream, by the caller -- and `capacity` the number of clouds
    the calls inside are launched with.  Scopes do not nest."""
    live_lib()
    assert count.is_cuda and count.numel() == 1 and str(count.dtype) == "torch.int32"
    call("g4d_live_scope_begin", count.data_ptr(), int(capacity))
    try:
        yield
    finally:
        call("g4d_live_scope_end")


def _entry(name):
    """The loaded function behind an entry point's name: libg4d_hip.so's, or that of whichever further loaded library declares it."""
    L = lib()
    if name not in PROTOTYPES:
        for M, protos, _ in _more.values():
            if name in protos:
                return getattr(M, name)
    return getattr(L, name)


_TRACE = os.environ.get("G4D_TRACE_CALLS", "0") != "0"   # debugging: every C-ABI call with its integer / float arguments on stderr
_TIMED = None   # measurement: a list collecting (name, integer args, start event, end event) of every call (timed_calls)
_UNTIMED = ("g4d_tuning_set", "g4d_tuning_set_thread", "g4d_launch_group_begin", "g4d_live_scope_begin", "g4d_live_scope_end")   # host state only: nothing to put events around


class timed_calls:
    """with _lib.timed_calls() as t: ...; t.results() -> [(entry point, integer arguments, microseconds)] of every C-ABI call made inside,
    from HIP events recorded on the stream each call launched on (torch's current stream), i.e. the GPU time of the call's launches plus the
    gap to the next event (2-5 us).  bench.py builds its per-launch table and the `roofline` objects from it, live."""

    def __enter__(self):
        global _TIMED
        self._rec = []
        _TIMED = self._rec
        return self

    def __exit__(self, *exc):
        global _TIMED
        _TIMED = None
        return False

    def results(self):
        import torch
        torch.cuda.synchronize()
        return [(name, ints, e0.elapsed_time(e1) * 1e3) for name, ints, e0, e1 in self._rec]


def call(name, *args):
    """Invoke a C-ABI entry point; non-zero status -> G4DError (the reference would exit(-1))."""
    L = lib()
    fn = _entry(name)
    timed = _TIMED is not None and args and name not in _UNTIMED
    if _TRACE or timed:
        label, shown = name, tuple(a for a in args if isinstance(a, int) and not isinstance(a, bool) and abs(a) < (1 << 31))
        if name == "g4d_mlp_run":
            # tracing / timing tables name the kernel family behind the argument block and list its leading integers (mode, rows, K0, ...)
            # as the positional entry points did
            blk = args[1].contents if hasattr(args[1], "contents") else MlpArgs.from_address(args[1])
            label = _MLP_FAMILY_NAMES[args[0]] if blk.unknown_grid is None else "g4d_mlp_chain_cells_bf16"
            shown = (blk.mode, blk.rows, blk.K0, blk.ldx, blk.N, blk.P, blk.S, blk.C, blk.use_xyz, blk.n, blk.m, blk.C2, blk.C1, blk.nlayers, blk.pool)
            if _TRACE:
                print("g4d call g4d_mlp_run ->", label, *shown, file=sys.stderr)
        if _TRACE:
            print("g4d call", name, *[a for a in args if isinstance(a, (int, float)) and abs(a) < (1 << 31)], file=sys.stderr)
    if timed:
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        _TIMED.append((label, shown, e0, e1))
    else:
        rc = fn(*args)
    if rc != 0:
        raise G4DError(f"{name} failed with status {rc}: {L.g4d_last_error().decode(errors='replace')}")
    return rc


def host_array(ctype, values):
    """`values` as a host array of `ctype`, in the form the C ABI takes it: a void pointer -- which keeps the array alive as long as it lives itself."""
    return ctypes.cast((ctype * len(values))(*values), ctypes.c_void_p)


def workspace(nbytes, device):
    """Device scratch for a `*_ws_bytes` / `*_bytes` size query, for callers that only pass its pointer on: a uint8 tensor of the queried
    size, never fewer bytes than asked for and never empty (16 at the least, so that the pointer is not null)."""
    import torch
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def ver(t):
    """A tensor's version counter for cache keys, or None for an inference tensor (torch.inference_mode(): no counter is kept -- and no in-place
    update outside inference mode is possible either)."""
    try:
        return t._version
    except RuntimeError:
        return None


def stream_ptr():
    """The current torch HIP stream as a raw hipStream_t (reference: at::cuda::getCurrentCUDAStream())."""
    import torch
    return torch.cuda.current_stream().cuda_stream
