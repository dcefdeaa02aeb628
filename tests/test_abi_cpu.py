"""CPU: the ctypes binding of libwsmgmap.so is the header, for every name.  wsmgmap._abi derives its argtypes, restypes and the four
host-array descriptors from include/wsmgmap.h; this file reads the same header with a reader of its own (written differently on
purpose, so that the comparison is not the parser against itself) and compares every declared entry point and every field, offset and
size of the descriptors.  The parser's own cases run on small literal strings.  The sentences and constants of the header that
feature tests rely on are pinned at the end: this is the only test file that reads the header's text, beside the name check of
tests/test_host_cpu.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "wsmgmap.h")).read()

# ---- the test-side reader ---------------------------------------------------------------------------------------------------------
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}
SIZES = {ctypes.c_void_p: 8, ctypes.c_int: 4, ctypes.c_uint: 4, ctypes.c_float: 4, ctypes.c_double: 8, ctypes.c_int64: 8,
         ctypes.c_longlong: 8}


def _code(text):
    """The header without comments: a scan, character by character (no nesting in C comments)."""
    out, i = [], 0
    while i < len(text):
        if text.startswith("/*", i):
            i = text.index("*/", i) + 2
            out.append(" ")
        elif text.startswith("//", i):
            i = text.index("\n", i)
        else:
            out.append(text[i])
            i += 1
    return "".join(out)


def _kind(param):
    """The ctypes type the binding must give one C parameter or field declaration, `TYPE name`."""
    if "*" in param or param.startswith("wsmg_stream_t "):
        return ctypes.c_void_p
    ty = param.rsplit(None, 1)[0]
    for names, kind in ((("int", "int32_t"), ctypes.c_int), (("unsigned", "uint32_t"), ctypes.c_uint), (("float",), ctypes.c_float),
                        (("double",), ctypes.c_double), (("int64_t",), ctypes.c_int64), (("long long",), ctypes.c_longlong)):
        if ty in names:
            return kind
    raise AssertionError(f"a type the ABI does not use: {param!r}")


def _declarations():
    """name -> (return type as written, [parameter declarations as written, blanks collapsed]): every entry point starts a line."""
    found = {}
    for ret, name, params in re.findall(r"^(const char\*|int64_t|long long|int) (wsmg_[a-z0-9_]+)\(([^()]*)\);", _code(HEADER), re.M):
        assert name not in found, f"{name} is declared twice"
        found[name] = (ret, [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
    return found


def _typedefs():
    """struct name -> [(field, kind)] with `int a, b;` lists expanded."""
    found = {}
    for body, name in re.findall(r"typedef struct \{([^{}]*)\} (Wsmg[A-Za-z]+Desc);", _code(HEADER)):
        fields = []
        for line in body.split(";"):
            if line.strip():
                head, *rest = [w.strip() for w in line.split(",")]
                fields.append((head.split()[-1], _kind(head)))
                fields += [(w, _kind(head)) for w in rest]
        found[name] = fields
    return found


DECLS = _declarations()
TYPEDEFS = _typedefs()


def test_the_reader_sees_the_whole_header():
    """Every `wsmg_name(` that stands in the header's code (the name check of tests/test_host_cpu.py counts the same way, comments
    included) is one of the reader's declarations, and the four descriptors are there."""
    assert set(DECLS) == set(re.findall(r"\b(wsmg_[a-z0-9_]+)\s*\(", _code(HEADER))) and len(DECLS) >= 169
    assert sorted(TYPEDEFS) == ["WsmgAdamDesc", "WsmgColsumDesc", "WsmgCopyDesc", "WsmgRelayoutDesc"]


# ---- every entry point --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DECLS))
def test_binding_of_every_entry_point_is_its_declaration(name):
    from wsmgmap import _abi
    ret, params = DECLS[name]
    fn = getattr(_abi.lib(), name)
    assert list(fn.argtypes) == [_kind(p) for p in params], params
    assert fn.restype is RETURNS[ret]
    assert _abi._SIG[name] == list(fn.argtypes) and _abi._RESTYPE[name] is fn.restype


def test_binding_has_no_name_the_header_does_not_declare():
    from wsmgmap import _abi
    assert set(_abi._SIG) == set(_abi._RESTYPE) == set(_abi.exported_names()) == set(DECLS)


# ---- the four descriptors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("struct,bound,size", [("WsmgCopyDesc", "CopyDesc", 24), ("WsmgColsumDesc", "ColsumDesc", 24),
                                               ("WsmgAdamDesc", "AdamDesc", 40), ("WsmgRelayoutDesc", "RelayoutDesc", 48)])
def test_descriptor_layout_is_the_typedef_under_natural_alignment(struct, bound, size):
    """Fields in the header's order, each at the next multiple of its own size, the whole padded to its widest member (a 64-bit
    host: 8-byte pointers and long long, 4-byte int)."""
    from wsmgmap import _abi, optim
    cls = getattr(_abi, bound)
    assert issubclass(cls, ctypes.Structure) and cls.__name__ == struct
    fields = TYPEDEFS[struct]
    assert [(n, t) for n, t in cls._fields_] == fields
    at = 0
    for n, kind in fields:
        at = -(-at // SIZES[kind]) * SIZES[kind]
        assert getattr(cls, n).offset == at and getattr(cls, n).size == SIZES[kind] == ctypes.sizeof(kind), n
        at += SIZES[kind]
    widest = max(SIZES[k] for _, k in fields)
    assert ctypes.sizeof(cls) == -(-at // widest) * widest == size
    assert optim._AdamDesc is _abi.AdamDesc


def test_descriptor_field_names_are_the_ones_the_callers_write():
    assert [n for n, _ in TYPEDEFS["WsmgCopyDesc"]] == ["dst", "src", "bytes"]
    assert [n for n, _ in TYPEDEFS["WsmgColsumDesc"]] == ["x", "out", "rows", "cols"]
    assert [n for n, _ in TYPEDEFS["WsmgAdamDesc"]] == ["param", "grad", "exp_avg", "exp_avg_sq", "n"]
    assert [n for n, _ in TYPEDEFS["WsmgRelayoutDesc"]] == ["w_oihw", "w_ohwi", "w_ihwo", "O", "I", "KH", "KW", "I_pad", "reserved"]


# ---- the package's parser on literal strings ----------------------------------------------------------------------------------------
P, I, U, F, D, L64, LL = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double, ctypes.c_int64,
                          ctypes.c_longlong)


def test_parser_maps_every_type_of_its_table():
    from wsmgmap._abi import parse_header
    sig, ret, structs = parse_header(
        "int wsmg_a(const float* p, void* q, const WsmgCopyDesc* d, wsmg_stream_t s, int i, int32_t j, unsigned u, uint32_t v, float f,"
        " double g, int64_t k, long long l, unsigned* t, const int* m);\n"
        "int64_t wsmg_b(int64_t rows, int C);\nlong long wsmg_c(int n);\nconst char* wsmg_d(void);\nconst char *wsmg_e(void);\n")
    assert sig == {"wsmg_a": [P, P, P, P, I, I, U, U, F, D, L64, LL, P, P], "wsmg_b": [L64, I], "wsmg_c": [I], "wsmg_d": [], "wsmg_e": []}
    assert ret == {"wsmg_a": I, "wsmg_b": L64, "wsmg_c": LL, "wsmg_d": ctypes.c_char_p, "wsmg_e": ctypes.c_char_p}
    assert structs == {} and list(sig) == ["wsmg_a", "wsmg_b", "wsmg_c", "wsmg_d", "wsmg_e"]


def test_parser_reads_lists_over_lines_with_comments_and_skips_what_is_not_a_declaration():
    from wsmgmap._abi import parse_header
    sig, ret, _ = parse_header(
        "/* int wsmg_ghost(int a); */\n#ifndef X\n#define X (-1)   /* wsmg_macro(1); */\n#include <stdint.h>\n"
        "#ifdef __cplusplus\nextern \"C\" {\n#endif\ntypedef void* wsmg_stream_t;\nenum { WSMG_A = 0, WSMG_B = 1 };\n"
        "// int wsmg_line(int a);\n"
        "int wsmg_f(const float* depth, int B,\n"
        "           int32_t* lin_idx /* may be NULL */, float* out,   // the planes\n"
        "           wsmg_stream_t stream);\n"
        "#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert sig == {"wsmg_f": [P, I, P, P, P]} and ret == {"wsmg_f": I}


def test_parser_expands_field_lists_of_a_struct():
    from wsmgmap._abi import parse_header
    sig, _, structs = parse_header(
        "typedef struct {\n  const float* x;   /* [rows][cols] */\n  float* out;\n  int a, b;\n  long long n;\n} WsmgTDesc;\n"
        "int wsmg_t(const WsmgTDesc* descs, int n, wsmg_stream_t stream);\n")
    assert structs == {"WsmgTDesc": [("x", P), ("out", P), ("a", I), ("b", I), ("n", LL)]}
    assert sig == {"wsmg_t": [P, I, P]}


@pytest.mark.parametrize("text,names", [
    ("int wsmg_g(const float* x, size_t n);", "size_t n.*wsmg_g"),
    ("int wsmg_g(const float* x, int);", "wsmg_g"),                       # a parameter without a name: nothing to tell a type from
    ("int wsmg_g(const float* x, const int n);", "const int n.*wsmg_g"),
    ("size_t wsmg_h(int n);", "wsmg_h"),
    ("void wsmg_h(int n);", "wsmg_h"),
    ("int wsmg_h(int (*callback)(int));", "wsmg_h"),
    ("typedef struct { char tag; } WsmgTDesc;", "char tag.*WsmgTDesc"),
    ("typedef struct { float *a, *b; } WsmgTDesc;", "WsmgTDesc"),
], ids=["size_t", "unnamed", "const_value", "return_size_t", "return_void", "callback", "struct_char", "struct_pointer_list"])
def test_parser_refuses_what_is_outside_its_table(text, names):
    from wsmgmap._abi import WsmgError, parse_header
    with pytest.raises(WsmgError, match=names):
        parse_header(text)


def test_a_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    from wsmgmap import _abi
    gone = str(tmp_path / "include" / "wsmgmap.h")
    monkeypatch.setattr(_abi, "HEADER_PATH", gone)
    with pytest.raises(_abi.WsmgError, match=re.escape(gone)):
        _abi._read_header()


def test_the_header_is_the_checkouts():
    from wsmgmap import _abi
    assert os.path.samefile(_abi.HEADER_PATH, os.path.join(ROOT, "include", "wsmgmap.h"))


# ---- what feature tests rely on in the header's text --------------------------------------------------------------------------------
def test_declarations_the_feature_tests_name_read_as_they_did():
    for name in ("wsmg_map_fuse_retrieve", "wsmg_bev_project", "wsmg_lstm_state_fwd_chain", "wsmg_lstm_state_bwd_chain",
                 "wsmg_lstm_state_chain_workgroups", "wsmg_adam_step_multi_hyper", "wsmg_grad_norm_multi_hyper", "wsmg_grad_norm_multi",
                 "wsmg_adam_step_multi_guarded", "wsmg_attn_fp8_mfma_bwd", "wsmg_grad_report_multi", "wsmg_grad_stats_multi",
                 "wsmg_nav_rows", "wsmg_nav_accumulate", "wsmg_copy_multi_guarded", "wsmg_sem_confusion_f32", "wsmg_sem_confusion_bf16",
                 "wsmg_sem_scores"):
        assert DECLS[name][0] == "int", name
    assert DECLS["wsmg_attn_fp8_mfma_bwd"][1][-1].startswith("wsmg_stream_t ")
    guarded = DECLS["wsmg_copy_multi_guarded"][1]
    assert guarded[0].startswith("const WsmgCopyDesc*") and guarded[1].startswith("int ") and guarded[2].startswith("const float*")
    assert [("*" in p or p.startswith("wsmg_stream_t")) for p in guarded] == [True, False, True, True]


def test_header_says_what_the_one_launch_forms_and_the_hyper_record_promise():
    assert "bit-identical" in HEADER[HEADER.index("int wsmg_bev_project(") - 1500:HEADER.index("int wsmg_map_fuse_retrieve(")]
    # the hyper record's layout is documented next to the guard record's
    assert "{lr, beta1, beta2, eps, weight_decay, 0, 0, 0}" in HEADER and HEADER.index("guard[0] norm") < HEADER.index("{lr, beta1,")


def test_nav_constants_of_the_header_are_the_ones_python_and_the_yardstick_use():
    import nav_eval_util as nu
    from wsmgmap import ops
    consts = {k: int(v) for k, v in re.findall(r"\b(WSMG_NAV_[A-Z0-9_]+)\s*=?\s+(\d+)\b", HEADER)}
    assert consts["WSMG_NAV_ROW"] == ops.NAV_ROW == nu.R and consts["WSMG_NAV_COUNTS"] == ops.NAV_COUNTS == 13
    assert consts["WSMG_NAV_SUMS"] == ops.NAV_SUMS == len(ops.NAV_SUM_FIELDS) == len(nu.SUM_FIELDS) == 12
    for key, name in dict(att_state="ATT_STATE", att_target="ATT_TARGET", att_peak="ATT_PEAK", att_cheb="ATT_CHEB", att_euclid="ATT_EUCLID",
                          att_mass="ATT_MASS", att_entropy="ATT_ENTROPY", act_state="ACT_STATE", act_sq="ACT_SQ", act_l2="ACT_L2",
                          act_abs="ACT_ABS", prog_state="PROG_STATE", prog_abs="PROG_ABS", prog_sq="PROG_SQ", prog_stop="PROG_STOP").items():
        assert consts["WSMG_NAV_" + name] == ops.NAV_FIELDS[key] == getattr(nu, name), name
    assert tuple(ops.NAV_SUM_FIELDS) == tuple(nu.SUM_FIELDS)
    assert (consts["WSMG_NAV_ABSENT"], consts["WSMG_NAV_COUNTED"], consts["WSMG_NAV_INVALID"]) == (0, 1, 2)
