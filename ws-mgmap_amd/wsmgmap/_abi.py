"""ctypes binding of libwsmgmap.so (C ABI declared in include/wsmgmap.h).

This is the only place the shared library is touched.  There is NO fallback: if the
library is missing, or a call returns non-zero, a WsmgError is raised — the product path
never silently degrades to PyTorch or CPU code.

No signature is written here: argtypes, restypes and the descriptor structures are read from the header's declarations, which
the compiler holds to the definitions (every .hip file includes the header).  A new entry point needs nothing in this file.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libwsmgmap.so")
if os.environ.get("WSMG_LIB"):       # experiments only: another build of the same library (read once, here)
    LIB_PATH = os.environ["WSMG_LIB"]
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "wsmgmap.h")   # the checkout's; also for a WSMG_LIB


class WsmgError(RuntimeError):
    pass


# The binding is derived from the header: the closed tables of the types the ABI uses.  Anything else is an error, never a guess.
_VALUE_TYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint,
                "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong,
                "wsmg_stream_t": ctypes.c_void_p}
_RETURN_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}


def _ctype(decl, where):
    """The ctypes type of one `TYPE name` declaration: every pointer is a void pointer, a value type comes from the table."""
    if "*" in decl:
        return ctypes.c_void_p
    ty = " ".join(decl.split()[:-1])
    if ty not in _VALUE_TYPES:
        raise WsmgError(f"{HEADER_PATH}: `{decl}` in {where} has a type outside the binding's table {sorted(_VALUE_TYPES)}")
    return _VALUE_TYPES[ty]


def parse_header(text):
    """(name -> argtypes, name -> restype, struct name -> ctypes fields) of every `RET wsmg_name(PARAMS);` and every
    `typedef struct { ... } Name;` of a header written as include/wsmgmap.h is."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = structs[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = (d.strip() for d in decl.split(","))          # `int rows, cols`: the names after the first share its type
            if "*" in decl and more:
                raise WsmgError(f"{HEADER_PATH}: `{decl}` in {name} declares several pointers at once")
            fields += [(n.split()[-1].lstrip("*"), _ctype(first, name)) for n in [first] + more]
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    sig, restype = {}, {}
    for stmt in text.split(";"):
        if "(" not in stmt:
            continue                                                     # extern "C" {, typedef void* wsmg_stream_t, }
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(wsmg_\w+)\s*\(([^()]*)\)\s*", stmt)
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split())) if m else None
        if ret not in _RETURN_TYPES:
            raise WsmgError(f"{HEADER_PATH}: `{' '.join(stmt.split())}` is not a declaration returning one of {sorted(_RETURN_TYPES)}")
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        sig[m.group(2)] = [] if params == ["void"] else [_ctype(p, m.group(2)) for p in params]
        restype[m.group(2)] = _RETURN_TYPES[ret]
    return sig, restype, structs


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise WsmgError(f"{HEADER_PATH} not found: the binding of libwsmgmap.so is derived from the checkout's header, "
                        "there is no second copy of the ABI")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> argtypes, name -> restype and the host-array descriptors, all as include/wsmgmap.h declares them
_SIG, _RESTYPE, _STRUCTS = _read_header()
CopyDesc, RelayoutDesc, ColsumDesc, AdamDesc = (type(n, (ctypes.Structure,), {"_fields_": _STRUCTS[n]})
                                                for n in ("WsmgCopyDesc", "WsmgRelayoutDesc", "WsmgColsumDesc", "WsmgAdamDesc"))

_lib = None


def lib():
    """The loaded library; raises WsmgError (never falls back) if it cannot be loaded."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WsmgError(
                f"{LIB_PATH} not found: build it with `make -C ws-mgmap_amd/csrc` "
                "(or __graft_entry__.build()). The HIP kernels are mandatory; there is no fallback path.")
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise WsmgError(f"cannot load {LIB_PATH}: {e}") from e
        for name, args in _SIG.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise WsmgError(f"{LIB_PATH} does not export {name}") from e
            fn.argtypes = args
            fn.restype = _RESTYPE[name]
        info = L.wsmg_build_info() or b""
        if b"rnn-nopk" not in info:
            # the GRU / LSTM gradient kernels are only correct when wsmg_rnn.hip was compiled without packed-fp32 instructions
            # (csrc/Makefile: EXTRA_wsmg_rnn; 177 wrong tensors in 60 loaded repeats otherwise): a stale object or another build
            # of the library (WSMG_LIB) must not bring that back silently
            raise WsmgError(f"{LIB_PATH} ({info.decode(errors='replace')}) was not built with the RNN kernels' compiler flags "
                            "(no 'rnn-nopk' in wsmg_build_info()): rebuild with `make -C ws-mgmap_amd/csrc`")
        _lib = L
    return _lib


def call(name, *args):
    """Call an int-returning entry point; non-zero is an error."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        kind = {-1: "WSMG_EINVAL (rejected arguments)", -2: "WSMG_ENOMEM (workspace too small)"}.get(rc, f"hipError_t {rc}")
        raise WsmgError(f"{name} failed: {kind}")


rnn_timeouts = 0      # persistent-RNN timeouts reported so far in this process


# Under a process group an exception that ONE rank raises between two collectives leaves its peers blocked in theirs.  While a
# GradAllReducer is active the forward pass's status checks therefore do nothing (`defer_rnn_status`); the reducer's `finish()`
# reads the word (force=True) and the ranks agree on the error before any of them raises (wsmgmap/parallel.py).
defer_rnn_status = False

STATUS_BITS = ((1, "gru_fwd"), (2, "gru_bwd"), (4, "lstm_fwd"), (8, "lstm_bwd"), (16, "attn_fp8_fused barrier"), (32, "lstm_state_fwd"),
               (64, "lstm_state_bwd"), (128, "instr_rnn_fwd"), (256, "instr_rnn_bwd"))


def check_rnn_status(sync=False, force=False):
    """Raise WsmgError if a persistent RNN kernel reported a timeout since the last check.  Reads a word in host-mapped
    pinned memory: no device synchronisation by itself.  Called at the host's natural sync points (the instruction dedup
    read-back of every forward pass, GradAllReducer.finish(), the end of an update in bench / tests) — those see every kernel
    that had FINISHED by then, so a timeout of the current update can surface one update late.  sync=True waits for the device
    first: the exact form, for a trainer that wants the guarantee that NaN-filled outputs never reach optimizer.step()
    (`BasePolicy.check_status()`).  force: also while a GradAllReducer defers the checks (its own call)."""
    global rnn_timeouts
    if defer_rnn_status and not force:
        return
    if sync:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    v = lib().wsmg_rnn_status(1)
    if v:
        rnn_timeouts += 1       # (owners of persistent, never-cleared RNN workspaces re-zero them: the error word in them is sticky)
        names = [n for b, n in STATUS_BITS if v & b]
        raise WsmgError("persistent kernel(s) timed out waiting for their cooperating workgroups: " + ", ".join(names) +
                        " — their outputs were filled with NaN; results since the previous check are invalid "
                        "(the persistent kernels need all their workgroups resident at once: too many concurrent persistent "
                        "kernels for the free CUs?  net.recurrent_chunks = 0 runs one at a time)")


def take_rnn_status():
    """The status word's bits since the last read, cleared, WITHOUT raising (0: nothing timed out) — for callers that handle a
    timeout themselves (bench.py's in-process fallback).  Counts as a reported timeout for the owners of never-cleared workspaces."""
    global rnn_timeouts
    v = int(lib().wsmg_rnn_status(1))
    if v:
        rnn_timeouts += 1
    return v


def status_names(bits):
    return [n for b, n in STATUS_BITS if bits & b]


def exported_names():
    return list(_SIG)
