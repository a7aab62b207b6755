"""ctypes binding of csrc/libkdiff_hip.so (C ABI declared in include/kdiff_hip.h).

There is NO fallback: if the shared library is missing or a symbol is absent, the first use raises.
The library is built in-tree by ``__graft_entry__.build()`` / ``make -C k-diffusion_amd/csrc``.
"""
import ctypes as C
import os

from ._abi import HeaderError, parse

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KDIFF_HIP_LIB") or os.path.join(_HERE, "csrc", "libkdiff_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "kdiff_hip.h")
GRAD_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "kdiff_unet_grad.h")
TRAIN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "kdiff_unet_train.h")
DROP_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "kdiff_unet_drop.h")
MIXED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "kdiff_unet_mixed.h")
UNET_BF16_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "kdiff_unet_bf16.h")


class NativeLibraryError(RuntimeError):
    pass


# The header is the one declaration of the ABI: every entry point's argument and return types (SIGNATURES, RESTYPES), the descriptor
# structs (KdGemm, KdFfn, KdCall, KdMtTensor, KdAdamGroup) and every KD_X enum constant / integer #define as X (A_PLAIN, EPI_QKV,
# STEP_TO_D, MT_CHUNK, OP_GEMM_F32, ...) are read from it here (_abi.parse states the type rule)
try:
    with open(HEADER_PATH) as _header:
        _parsed = parse(_header.read())
except OSError as e:
    raise NativeLibraryError(f"{HEADER_PATH}: the C ABI header the package binds from cannot be read ({e})") from e
SIGNATURES, RESTYPES = _parsed.signatures, _parsed.restypes
globals().update(_parsed.structs)
globals().update({name[3:]: value for name, value in _parsed.constants.items()})
# entry points a kd_run_list entry can name: KD_OP_X names kd_x
RUN_LIST_OPS = {"kd_" + name[6:].lower(): value for name, value in _parsed.constants.items() if name.startswith("KD_OP_")}
if not set(RUN_LIST_OPS) <= set(SIGNATURES):
    raise HeaderError(f"KD_OP_* without an entry point: {sorted(set(RUN_LIST_OPS) - set(SIGNATURES))}")
# The U-Net's reverse kernels (csrc/unet_vjp_f32.hip) are declared in a header of their own, read by the same parser into a table of their
# own: prototypes only, and no kd_run_list entry can name them
try:
    with open(GRAD_HEADER_PATH) as _header:
        _grad = parse(_header.read())
except OSError as e:
    raise NativeLibraryError(f"{GRAD_HEADER_PATH}: the C ABI header the package binds from cannot be read ({e})") from e
if _grad.structs or _grad.constants or set(_grad.signatures) & set(SIGNATURES):
    raise HeaderError(f"{GRAD_HEADER_PATH}: prototypes of entry points kdiff_hip.h does not declare, and nothing else")
GRAD_SIGNATURES, GRAD_RESTYPES = _grad.signatures, _grad.restypes
# ... and so are its parameter-gradient kernels (csrc/conv_wgrad_x3.hip, csrc/unet_train_f32.hip): a third header, a third table
try:
    with open(TRAIN_HEADER_PATH) as _header:
        _train = parse(_header.read())
except OSError as e:
    raise NativeLibraryError(f"{TRAIN_HEADER_PATH}: the C ABI header the package binds from cannot be read ({e})") from e
if _train.structs or _train.constants or set(_train.signatures) & (set(SIGNATURES) | set(GRAD_SIGNATURES)):
    raise HeaderError(f"{TRAIN_HEADER_PATH}: prototypes of entry points the other two headers do not declare, and nothing else")
TRAIN_SIGNATURES, TRAIN_RESTYPES = _train.signatures, _train.restypes
# ... and its dropout kernels (csrc/unet_drop_f32.hip, one entry point each in csrc/conv_x3.hip and two in csrc/vjp_f32.hip): a fourth header, a fourth table
try:
    with open(DROP_HEADER_PATH) as _header:
        _drop = parse(_header.read())
except OSError as e:
    raise NativeLibraryError(f"{DROP_HEADER_PATH}: the C ABI header the package binds from cannot be read ({e})") from e
if _drop.structs or _drop.constants or set(_drop.signatures) & (set(SIGNATURES) | set(GRAD_SIGNATURES) | set(TRAIN_SIGNATURES)):
    raise HeaderError(f"{DROP_HEADER_PATH}: prototypes of entry points the other three headers do not declare, and nothing else")
DROP_SIGNATURES, DROP_RESTYPES = _drop.signatures, _drop.restypes
# ... and the bf16 form of its convolution weight gradient (csrc/conv_wgrad_bf16.hip): a fifth header, a fifth table
try:
    with open(MIXED_HEADER_PATH) as _header:
        _mixed = parse(_header.read())
except OSError as e:
    raise NativeLibraryError(f"{MIXED_HEADER_PATH}: the C ABI header the package binds from cannot be read ({e})") from e
if _mixed.structs or _mixed.constants or set(_mixed.signatures) & (set(SIGNATURES) | set(GRAD_SIGNATURES) | set(TRAIN_SIGNATURES) | set(DROP_SIGNATURES)):
    raise HeaderError(f"{MIXED_HEADER_PATH}: prototypes of entry points the other four headers do not declare, and nothing else")
MIXED_SIGNATURES, MIXED_RESTYPES = _mixed.signatures, _mixed.restypes
# ... and the bf16 form of its sampling forward's convolution (csrc/conv_bf16.hip): a sixth header, a sixth table
try:
    with open(UNET_BF16_HEADER_PATH) as _header:
        _unet_bf16 = parse(_header.read())
except OSError as e:
    raise NativeLibraryError(f"{UNET_BF16_HEADER_PATH}: the C ABI header the package binds from cannot be read ({e})") from e
if _unet_bf16.structs or _unet_bf16.constants or set(_unet_bf16.signatures) & (set(SIGNATURES) | set(GRAD_SIGNATURES) | set(TRAIN_SIGNATURES)
                                                                               | set(DROP_SIGNATURES) | set(MIXED_SIGNATURES)):
    raise HeaderError(f"{UNET_BF16_HEADER_PATH}: prototypes of entry points the other five headers do not declare, and nothing else")
UNET_BF16_SIGNATURES, UNET_BF16_RESTYPES = _unet_bf16.signatures, _unet_bf16.restypes
_i, _f = C.c_int, C.c_float                  # the kinds encode_call tells apart (the parser hands out these very objects)

# PREC_FP8 is a mode of the NETWORK, not a KdGemm.precision value: the bf16 mode with the AdaRMSNorm -> wide projections of the K = 256 / 512
# levels on the block-scaled fp8 matrix instruction (kd_gemm_mx8); every descriptor of such a plan says KD_PREC_BF16
PREC_FP8 = 3
_MODES = {"exact": PREC_EXACT, "split3": PREC_SPLIT3, "bf16": PREC_BF16, "fp8": PREC_FP8}


def default_precision():
    """Arithmetic mode of the network (KDIFF_GEMM):
    exact   fp32-input MFMA, bit-for-bit an fmaf chain (fp32 activations);
    split3  (default) every fp32 operand split into two bf16, 3 bf16 MFMAs per product, fp32 accumulate (fp32 activations):
            the fp32-parity mode, inside the 1e-3 tolerance of the reference's fp32 path;
    bf16    bf16 activations in HBM, one bf16 MFMA per product, fp32 accumulate / statistics / softmax: the arithmetic of the
            reference under torch.autocast(bfloat16);
    fp8     the bf16 mode with the norm -> qkv / norm -> GEGLU projections of the K = 256 / 512 levels as e4m3 x e4m3 products with
            power-of-two block scales (weights per output channel, activations per 32-k block) on the fp8 matrix instruction."""
    mode = os.environ.get("KDIFF_GEMM", "split3").lower()
    if mode not in _MODES:
        raise ValueError(f"KDIFF_GEMM={mode!r}: expected one of {sorted(_MODES)}")
    return _MODES[mode]


def kernel_precision():
    """KdGemm.precision of the default mode: the fp8 mode's descriptors are bf16 descriptors (see PREC_FP8)."""
    p = default_precision()
    return PREC_BF16 if p == PREC_FP8 else p


def precision_name(p):
    return {v: k for k, v in _MODES.items()}[p]


def encode_call(call, name, args):
    """Fill the KdCall ``call`` from an entry point's name and its positional arguments WITHOUT the trailing stream: pointers (None, int
    addresses, c_void_p, or a ctypes Structure = its address) go to ``p`` in order, ints to ``i`` in order, the float to ``f`` -- the rule
    kd_run_list unpacks by.  An argument with a ``bind_call(call, index)`` method (a pointer the caller patches per run) is told where it
    lives.  Returns False if the entry point cannot be named in a list."""
    op = RUN_LIST_OPS.get(name)
    if op is None:
        return False
    kinds = SIGNATURES[name][:-1]
    if len(kinds) != len(args):
        raise ValueError(f"{name}: {len(args)} arguments for {len(kinds)} parameters")
    call.op = op
    n_p = n_i = 0
    for kind, a in zip(kinds, args):
        if kind is _i:
            call.i[n_i] = int(a)
            n_i += 1
        elif kind is _f:
            call.f = a.value if isinstance(a, C.c_float) else float(a)
        else:
            if hasattr(a, "bind_call"):
                a.bind_call(call, n_p)
                v = a.scale
            elif isinstance(a, C.Structure):
                v = C.addressof(a)
            elif isinstance(a, C.c_void_p):
                v = a.value
            else:
                v = a
            call.p[n_p] = v
            n_p += 1
    return True

_lib = None


def lib():
    """The loaded shared library (loads on first use; raises loudly if it is not there)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C k-diffusion_amd/csrc). "
                "There is no CPU / PyTorch fallback for the sampling hot path.")
        handle = C.CDLL(LIB_PATH)
        for signatures, restypes in ((SIGNATURES, RESTYPES), (GRAD_SIGNATURES, GRAD_RESTYPES), (TRAIN_SIGNATURES, TRAIN_RESTYPES),
                                     (DROP_SIGNATURES, DROP_RESTYPES), (MIXED_SIGNATURES, MIXED_RESTYPES),
                                     (UNET_BF16_SIGNATURES, UNET_BF16_RESTYPES)):
            for name, argtypes in signatures.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError as e:
                    raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
                fn.argtypes = argtypes
                fn.restype = restypes[name]
        _lib = handle
    _sync_options(_lib)
    return _lib


# The library reads no environment variables; KDIFF_OPTIONS="name=value,..." is mapped onto kd_set_option here (re-read whenever it changes,
# so that tests can flip options inside one process).
_env_applied = None       # (KDIFF_OPTIONS, {name: value} parsed from it) as last applied
_programmatic = set()     # option names set through set_option(): the environment sync leaves them alone
OPTION_DEFAULT = -2 ** 31  # INT_MIN: kd_set_option goes back to the built-in default, kd_get_option returns it (include/kdiff_hip.h)
option_epoch = 0          # bumped whenever a library option may have changed: captured launch graphs are bound to one epoch


def _parse_options(text):
    out = {}
    for item in (text or "").split(","):
        if item.strip():
            name, _, val = item.partition("=")
            out[name.strip()] = int(val)
    return out


def _sync_options(handle):
    """KDIFF_OPTIONS="name=value,..." sets any library option by name (A-B runs of bench.py).  Only what CHANGED since the last call is
    re-applied: an entry that changed or appeared, and -- reset to the library default -- an entry that disappeared.  Options set
    through ``set_option`` are not touched unless the environment names them anew."""
    global _env_applied, option_epoch
    raw = os.environ.get("KDIFF_OPTIONS")
    if _env_applied is not None and raw == _env_applied[0]:
        return
    named = _parse_options(raw)
    old_named = _env_applied[1] if _env_applied is not None else {}
    for name, val in named.items():
        if old_named.get(name) != val:
            if handle.kd_set_option(name.encode(), val) != 0:
                raise ValueError(f"KDIFF_OPTIONS: unknown library option {name!r}")
            _programmatic.discard(name)
    for name in old_named:
        if name not in named and name not in _programmatic:
            handle.kd_set_option(name.encode(), OPTION_DEFAULT)
    _env_applied = (raw, named)
    option_epoch += 1


prof_active = False


def prof_enable(on):
    """Per-launch HIP-event timing of every kernel (kd_prof_*).  While it is on, the model issues its launch lists directly
    (a captured graph has no per-kernel events to read back)."""
    global prof_active
    check(lib().kd_prof_enable(1 if on else 0), "kd_prof_enable")
    prof_active = bool(on)


def set_option(name, value):
    """Tuning / A-B switch of the library (include/kdiff_hip.h: kd_set_option)."""
    global option_epoch
    check(lib().kd_set_option(name.encode(), int(value)), "kd_set_option")
    _programmatic.add(name)
    option_epoch += 1


def check(code, what="libkdiff_hip"):
    if code != 0:
        msg = lib().kd_last_error()
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else '?'}")
