"""CPU: the policy option MODEL.TEXT_ATTENTION ("f32" default, "fp8": ops.attention_fp8_shared in both directions) and the C ABI of
the shared-set fp8 attention's backward (wsmg_attn_fp8_mfma_bwd): declared, exported, and refusing invalid arguments with WSMG_EINVAL
before anything is enqueued.  The kernels are tested on the GPU (tests/test_gpu_attn_fp8_shared_bwd.py, test_gpu_fp8_text_attention.py)."""
import ctypes

import pytest

EINVAL = -1
NAME = "wsmg_attn_fp8_mfma_bwd"


class _Box:
    shape = (2,)


def test_text_attention_defaults_to_f32_and_accepts_fp8():
    from wsmgmap.config import default_model_config, text_attention_option
    cfg = default_model_config()
    assert cfg.TEXT_ATTENTION == "f32" and text_attention_option(cfg) == "f32"
    assert text_attention_option(default_model_config(text_attention="fp8")) == "fp8"
    del cfg["TEXT_ATTENTION"]                       # a reference config has no such field
    assert text_attention_option(cfg) == "f32"
    cfg["text_attention"] = "FP8"                   # both spellings, as COMPUTE_DTYPE; the upper-case field wins
    assert text_attention_option(cfg) == "fp8"
    cfg["TEXT_ATTENTION"] = "f32"
    assert text_attention_option(cfg) == "f32"


def test_text_attention_int8_is_a_value_error():
    from wsmgmap.config import default_model_config, text_attention_option
    from wsmgmap.models.policy import BasePolicy
    with pytest.raises(ValueError, match="TEXT_ATTENTION"):
        text_attention_option(default_model_config(text_attention="int8"))
    with pytest.raises(ValueError, match="TEXT_ATTENTION"):
        BasePolicy(None, _Box(), default_model_config(text_attention="int8"))


def test_policy_carries_the_option_and_the_recurrent_gate_refuses_fp8():
    import torch
    from wsmgmap import recurrent
    from wsmgmap.config import default_model_config
    from wsmgmap.fallback import RecurrentCoreFallback
    from wsmgmap.models.policy import BasePolicy
    assert BasePolicy(None, _Box(), default_model_config()).net.text_attention == "f32"
    pol = BasePolicy(None, _Box(), default_model_config(text_attention="fp8"))
    assert pol.net.text_attention == "fp8"
    rep = RecurrentCoreFallback(pol, verbose=False).report()
    assert rep["recurrent_core"].startswith("staged") and "TEXT_ATTENTION" in rep["recurrent_core"], rep
    # the gate itself (no device needed to be refused: the option is the first condition)
    x = torch.zeros(8, 16)
    assert recurrent.usable(x, torch.zeros(8, 4, 256), 2, (x, x), text_attention="fp8") is False


def test_backward_entry_point_is_declared_and_exported():
    """(Every argument against the header's declaration, the stream last: tests/test_abi_cpu.py.)"""
    from wsmgmap import _abi
    assert len(_abi._SIG[NAME]) == 22 and _abi._RESTYPE[NAME] is ctypes.c_int
    assert NAME in _abi.exported_names()


def _call(lib, **over):
    """wsmg_attn_fp8_mfma_bwd on host buffers that are never dereferenced: every case below must be refused before a launch."""
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(q_codes=p, q_scale=p, k_codes=p, k_scale=p, v_codes=p, v_scale=p, row_ids=p, set_start=p, inverse=p, attn=p, dout=p, dattn=p,
             scale=1.0 / 16, B=4, U=2, L=8, C=256, dq=p, dk=p, dv=p, dl_scratch=p, stream=None)
    a.update(over)
    return getattr(lib, NAME)(*a.values())


@pytest.mark.parametrize("over", [dict(C=128), dict(C=512), dict(L=225), dict(L=0), dict(B=0), dict(U=0), dict(U=1025), dict(dq=None),
                                  dict(dk=None), dict(dv=None), dict(dl_scratch=None), dict(attn=None), dict(inverse=None),
                                  dict(row_ids=None), dict(set_start=None), dict(q_codes=None), dict(k_scale=None), dict(v_codes=None)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_backward_entry_point_refuses_invalid_arguments(over):
    from wsmgmap import _abi
    try:
        lib = _abi.lib()
    except _abi.WsmgError as e:          # the library needs a GPU runtime this machine cannot load
        pytest.skip(str(e)[:120])
    assert _call(lib, **over) == EINVAL
