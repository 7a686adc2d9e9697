"""The extension's Python surface (csrc/bindings.cpp): the names it exports, that every call site in the package
resolves against the binding's own signature, and that bad arguments are rejected before any launch. Needs the
built extension; launches nothing."""
import ast
import os
import re

import pytest

import dbx_distributed_pytorch_examples_amd as pkg
from dbx_distributed_pytorch_examples_amd.ops import _ext

pytestmark = pytest.mark.skipif(not _ext.available(), reason="native extension not built")

PKG = os.path.dirname(os.path.abspath(pkg.__file__))
CALLERS = ("ops/kernels.py", "engine/native_mnist.py", "parallel/comm.py", "data/mds.py")

# the module's public names before the bindings were derived from csrc/entry.h: 80
NAMES = """MDSReader adam arch augment_mix_u8 augment_u8 avgpool_bwd avgpool_fwd bn_apply bn_bwd_apply bn_bwd_apply2
bn_bwd_coeff bn_bwd_reduce bn_eval_coeff bn_eval_coeff_multi bn_finalize cast_f32_bf16 ce_eval channel_stats
clip_factor colsum comm_abort comm_all_gather comm_all_reduce comm_async_error comm_available comm_broadcast
comm_config_supported comm_destroy comm_group_end comm_group_start comm_init comm_origin comm_rank
comm_reduce_scatter comm_set_timeout comm_size comm_unique_id comm_version conv_dwfused conv_igemm conv_wgrad
crop_resize_u8 dar_alloc dar_free dar_host_err dar_launch dar_launch_multi dar_max_ranks dar_read_err dropout
ema_update ema_update_multi grad_accum ipc_close ipc_handle ipc_open lamb lars_scale maxpool_bwd maxpool_fwd
mnist_bwd mnist_fwd mnist_saved_bytes normalize_u8 pool_bn_bwd sgd small_gemm softmax_ce stem_bwd sumsq
ta_apply_u8 ta_prepare weight_prep weight_prep16 wgrad_patch3 wgrad_reduce wgrad_reduce_gather
wgrad_reduce_job_bytes wgrad_reduce_multi_plan wgrad_reduce_multi_run""".split()


def signature(name):
    """[(parameter name, has a default)] from the first line of a binding's docstring; None for what is not
    one plain function (a class, an attribute)."""
    obj = getattr(_ext.C(), name)
    doc = getattr(obj, "__doc__", None) or ""
    m = re.match(rf"{name}\((.*)\) -> ", doc.splitlines()[0]) if doc and not isinstance(obj, (type, str)) else None
    if m is None:
        return None
    params, depth, cur = [], 0, ""
    for ch in m.group(1):
        depth += ch in "[(" and 1 or ch in "])" and -1 or 0
        if ch == "," and depth == 0:
            params.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        params.append(cur)
    return [(p.split(":")[0].strip(), " = " in p) for p in params]


def _is_ext(node, local_ext):
    """Is ``node`` the extension module: ``C()``, ``_C()``, ``self._C`` or a local name bound to one of them?"""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ("C", "_C"):
        return not node.args and not node.keywords
    if isinstance(node, ast.Attribute) and node.attr == "_C":
        return isinstance(node.value, ast.Name) and node.value.id == "self"
    return isinstance(node, ast.Name) and node.id in local_ext


def ext_calls():
    """(file, function node or None, call node, entry name) of every call into the extension in CALLERS."""
    out = []
    for rel in CALLERS:
        tree = ast.parse(open(os.path.join(PKG, rel)).read())
        scopes = [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]
        seen = set()
        for scope in scopes + [tree]:  # innermost functions first is not needed: a call is reported once
            local_ext = {t.id for n in ast.walk(scope) if isinstance(n, ast.Assign) and _is_ext(n.value, ())
                         for t in n.targets if isinstance(t, ast.Name)}
            for n in ast.walk(scope):
                if (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and _is_ext(n.func.value, local_ext)
                        and id(n) not in seen):
                    seen.add(id(n))
                    out.append((rel, scope if scope is not tree else None, n, n.func.attr))
    return out


def _dict_keys(node):
    """Keys of a ``dict(k=...)`` / ``{"k": ...}`` / ``dict(zip(NAMES, ...))`` expression; None if it is none of them."""
    if isinstance(node, ast.Dict):
        return [k.value for k in node.keys]
    if isinstance(node, ast.IfExp):
        a, b = _dict_keys(node.body), _dict_keys(node.orelse)
        return None if a is None or b is None else a + b
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "dict":
        if node.args and isinstance(node.args[0], ast.Call) and getattr(node.args[0].func, "id", "") == "zip":
            from dbx_distributed_pytorch_examples_amd.ops import kernels
            return list(getattr(kernels, node.args[0].args[0].id))
        return [k.arg for k in node.keywords]
    return None


def test_public_names_are_the_parents():
    assert sorted(n for n in dir(_ext.C()) if not n.startswith("_")) == sorted(NAMES)
    assert len(NAMES) == 80


def test_call_sites_resolve_against_the_signatures():
    calls = ext_calls()
    assert {c[0] for c in calls} == set(CALLERS) and len(calls) >= 60
    named = 0
    for rel, scope, call, name in calls:
        where = f"{rel}:{call.lineno} {name}"
        assert hasattr(_ext.C(), name), where
        sig = signature(name)
        if sig is None:
            continue
        names = [p for p, _ in sig]
        kws = [k.arg for k in call.keywords if k.arg is not None]
        assert set(kws) <= set(names), (where, set(kws) - set(names))
        named += bool(kws)
        splat = any(isinstance(a, ast.Starred) for a in call.args) or any(k.arg is None for k in call.keywords)
        assert len(call.args) + len(kws) <= len(names), where
        if not splat:
            given = set(names[:len(call.args)]) | set(kws)
            assert len(given) == len(call.args) + len(kws), where  # nothing given twice
            assert {p for p, d in sig if not d} <= given, (where, {p for p, d in sig if not d} - given)
        for k in call.keywords:  # ``**name``: every dict the enclosing function binds to that name
            if k.arg is None:
                assert isinstance(k.value, ast.Name) and scope is not None, where
                vals = [n.value for n in ast.walk(scope) if isinstance(n, ast.Assign)
                        and any(isinstance(t, ast.Name) and t.id == k.value.id for t in n.targets)]
                assert vals, where
                for v in vals:
                    keys = _dict_keys(v)
                    if keys is None:  # the one dict a method builds: BNBwdEpilogue.args()
                        assert isinstance(v, ast.Call) and v.func.attr == "args", (where, ast.dump(v))
                        from dbx_distributed_pytorch_examples_amd.ops.kernels import MASK_Y, BNBwdEpilogue
                        keys = list(BNBwdEpilogue(MASK_Y, None, None, None, None).args())
                    assert set(keys) <= set(names) and not set(keys) & set(kws), (where, keys)
    assert named >= 10  # the struct-filling entries' ten call sites


def _igemm(**kw):
    base = dict(mode=0, bm=128, bn=128, x=0, w=0, y=0, nshard=1, N=1, IH=1, IW=1, IC=64, OH=1, OW=1, OC=64, R=1, S=1,
                stride=1, pad=0, nr=1, ns=1, r0=0, s0=0, FH=1, FW=1, st=0, dma=0)
    return _ext.C().conv_igemm(**{**base, **kw})


def test_validations_throw_before_the_launch():
    c = _ext.C()
    with pytest.raises(ValueError, match="input finalize without a BN prologue"):
        _igemm(fin_in=1)
    with pytest.raises(ValueError, match="BN finalize without statistics"):
        _igemm(fin1=1)
    with pytest.raises(ValueError, match="second BN finalize without its statistics"):
        _igemm(fin2=1, bstats1=1)
    with pytest.raises(ValueError, match="fused split-K reduction needs tile counters"):
        c.conv_wgrad(mode=0, bm=64, bn=64, dy=0, x=0, ws=0, in_scale=0, in_shift=0, relu_in=0, N=1, IH=1, IW=1,
                     IC=64, OH=1, OW=1, OC=64, R=1, S=1, stride=1, pad=0, KTOT=64, nsplit=2, m_per_split=1,
                     st=0, lds_pad=0, dma=0, dw=1, scale=1.0, accumulate=0)
    with pytest.raises(RuntimeError, match="batch too large for mdiv"):
        c.stem_bwd(y=0, x4=0, ws=0, ws_cap=0, N=1 << 20, H=1 << 10, W=1 << 10, C=64, P=0, Q=0, PK=0, pstride=1,
                   ppad=0, IH=1, IW=1, R=7, S=7, stride=2, pad=3, st=0)
    with pytest.raises(ValueError, match="job lists of different lengths"):
        c.wgrad_reduce_multi_plan([0, 0], [0], [4, 4], [1, 1], [1.0, 1.0], [0, 0], 0)


def test_an_unknown_or_missing_keyword_is_a_type_error():
    with pytest.raises(TypeError):
        _igemm(no_such_field=1)
    with pytest.raises(TypeError):
        _ext.C().conv_igemm(mode=0, bm=128, bn=128)


def test_derived_bindings_reject_bad_arguments():
    c = _ext.C()
    sig = signature("wgrad_reduce")
    assert len(sig) == 7 and not any(d for _, d in sig)
    with pytest.raises(TypeError):
        c.wgrad_reduce(0, 0, 4, 1, 1.0, 0)  # the stream is missing
    with pytest.raises(TypeError):
        c.wgrad_reduce("ws", 0, 4, 1, 1.0, 0, 0)
    with pytest.raises(TypeError):
        c.normalize_u8(b"\0", 0, 0, 1, 1, 1, 3, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0)  # bytes are no pointer either


def test_host_only_entries_run():
    c = _ext.C()
    assert c.wgrad_reduce_job_bytes() == 48 and c.mnist_saved_bytes() > 0
    import numpy as np
    table = np.zeros(2 * c.wgrad_reduce_job_bytes(), dtype=np.uint8)
    ga, gb = c.wgrad_reduce_multi_plan([64, 128], [256, 512], [1024, 2048], [2, 16], [1.0, 0.5], [0, 1],
                                       table.ctypes.data)
    assert (ga, gb) == (8, 1 + 2)  # the 16-split job first sums 4 groups of 4 slabs; 256 / 512 float4 per job
    assert table[:16].view(np.int64).tolist() == [64, 256]
