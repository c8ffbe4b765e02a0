"""CPU: the prefill attention export (skv_prefill_attention) is declared, bound and refuses bad arguments on the host, before
any HIP call, so its checks run without a GPU: -1 = SKV_ERR_ARG, -2 = SKV_ERR_UNSUPPORTED."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prefill_export_is_declared_and_bound():
    from shadowkv_amd import _lib
    text = open(os.path.join(ROOT, "include", "shadowkv_hip.h")).read()
    assert re.search(r"SKV_EXPORT\s+int\s+skv_prefill_attention\s*\(", text)
    assert "skv_prefill_attention" in _lib.EXPORTS
    assert _lib.lib().skv_abi_version() == 1          # an additive export: the ABI version stays


def _call(**kw):
    from shadowkv_amd import _lib
    p = 0x1000                                          # a non-null pointer that is never dereferenced on the host
    a = dict(q=p, k=p, v=p, out=p, bs=1, hq=8, hkv=2, q_len=100, kv_len=100, d=128,
             qs=(8 * 100 * 128, 100 * 128, 128), ks=(2 * 100 * 128, 100 * 128, 128), vs=(2 * 100 * 128, 100 * 128, 128))
    a.update(kw)
    return _lib.lib().skv_prefill_attention(a["q"], a["k"], a["v"], a["out"], a["bs"], a["hq"], a["hkv"], a["q_len"],
                                             a["kv_len"], a["d"], *a["qs"], *a["ks"], *a["vs"], 0.088, 0)


def test_prefill_attention_refuses_bad_arguments_before_any_launch():
    assert _call(q=0) == -1
    assert _call(k=0) == -1
    assert _call(v=0) == -1
    assert _call(out=0) == -1
    assert _call(q_len=0) == -1                         # q_len < 1
    assert _call(kv_len=99) == -1                       # kv_len < q_len
    assert _call(hq=6, hkv=4) == -1                     # Hq % Hkv != 0
    assert _call(bs=0) == -1
    assert _call(qs=(8 * 100 * 128, 100 * 128, 132)) == -1     # row stride not 16-byte aligned
    assert _call(ks=(2 * 100 * 128, 100 * 128 + 4, 128)) == -1  # head stride not 16-byte aligned
    assert _call(vs=(2 * 100 * 128 + 2, 100 * 128, 128)) == -1  # batch stride not 16-byte aligned
    assert _call(out=0x1008) == -1                      # pointer not 16-byte aligned
    assert _call(d=64, qs=(8 * 100 * 64, 100 * 64, 64), ks=(2 * 100 * 64, 100 * 64, 64),
                 vs=(2 * 100 * 64, 100 * 64, 64)) == -2  # D != 128
    assert _call(d=256) == -2
