"""Shared by the tests that ask the bf16 conv engine which kernel a call takes (wsmg_conv_route_bf16): the header's constants and
the query as a dictionary.  No test here."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "wsmgmap.h")).read()
C = {k: int(v) for k, v in re.findall(r"\b(WSMG_(?:CONV|NEED|ROUTE|RW)_[A-Z0-9_]+) = (\d+)", _HEADER)}
WORDS = int(re.search(r"#define WSMG_ROUTE_WORDS (\d+)", _HEADER).group(1))
FWD, BWD_DATA, BWD_WEIGHT = C["WSMG_CONV_FWD"], C["WSMG_CONV_BWD_DATA"], C["WSMG_CONV_BWD_WEIGHT"]
F32, SLICE, RELU_Y, SPLIT, STATS = (C["WSMG_NEED_" + n] for n in ("F32", "SLICE", "RELU_Y", "SPLIT", "STATS"))
FAMILY = {v: k[len("WSMG_ROUTE_"):] for k, v in C.items() if k.startswith("WSMG_ROUTE_")}      # 0 -> "IGEMM", ...
FIELDS = {k[len("WSMG_RW_"):].lower(): v for k, v in C.items() if k.startswith("WSMG_RW_")}   # "kind" -> 0, ...


def dims(B, Cin, Cout, k, s, p, H, W=None):
    """The eleven geometry arguments of the conv entry points for a square kernel."""
    W = H if W is None else W
    return (B, H, W, Cin, Cout, k, k, s, p, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)


def route_rc(pass_, geom, needs=0):
    """(return code, route words as a dictionary with the family by name)."""
    from wsmgmap import _abi
    words = (ctypes.c_int * WORDS)(*([-7] * WORDS))
    rc = _abi.lib().wsmg_conv_route_bf16(pass_, *geom, needs, ctypes.cast(words, ctypes.c_void_p))
    r = {name: words[i] for name, i in FIELDS.items()}
    r["kind"] = FAMILY.get(r["kind"], r["kind"])
    return rc, r


def route(pass_, geom, needs=0):
    rc, r = route_rc(pass_, geom, needs)
    assert rc == 0, (pass_, geom, needs, rc)
    return r


def plan_nsplit(geom):
    """nsplit of wsmg_conv2d_bwd_weight_bf16_plan, its workspace size checked."""
    from wsmgmap import _abi
    ns, fl = ctypes.c_int(0), ctypes.c_longlong(0)
    _abi.call("wsmg_conv2d_bwd_weight_bf16_plan", *geom, ctypes.cast(ctypes.byref(ns), ctypes.c_void_p),
              ctypes.cast(ctypes.byref(fl), ctypes.c_void_p))
    B, H, W, Cin, Cout, KH, KW = geom[:7]
    assert fl.value == ns.value * Cout * KH * KW * Cin
    return ns.value
