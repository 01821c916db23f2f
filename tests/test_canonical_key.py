"""``_objcore.canonical`` / ``objutil.canonical_json``: byte for byte what
``json.dumps(obj, sort_keys=True, separators=(",", ":"))`` gives — it keys the cache of defaulted
pod specs (``utils/reconcilehelper._defaulted``) and feeds the StatefulSet template hash, so a
different byte would be a different key."""

from __future__ import annotations

import json
import random

import pytest

oc = pytest.importorskip("odh_kubeflow_amd.native._objcore")

from odh_kubeflow_amd.controllers.notebook import generate_statefulset  # noqa: E402
from odh_kubeflow_amd.models import defaults  # noqa: E402
from odh_kubeflow_amd.models.notebook import notebook  # noqa: E402
from odh_kubeflow_amd.testing.kubelet.statefulset import template_hash  # noqa: E402
from odh_kubeflow_amd.utils import reconcilehelper  # noqa: E402
from odh_kubeflow_amd.utils.objutil import canonical_json, deepcopy_json  # noqa: E402

CHARS = ["a", "Z", "0", " ", '"', "\\", "/", "\n", "\t", "\r", "\b", "\f", "\x00", "\x1f", "\x7f", "\x80", "é", "ÿ",
         "中", " ", "\ud800", "\U0001F600", "\U0010FFFF", "~", "<", "&"]


def _want(o) -> bytes:
    return json.dumps(o, sort_keys=True, separators=(",", ":")).encode()


def _text(rnd, n=10):
    return "".join(rnd.choice(CHARS) for _ in range(rnd.randrange(0, n)))


def _rand(rnd: random.Random, depth: int = 0):
    r = rnd.random()
    if depth > 4 or r < 0.35:
        k = rnd.randrange(8)
        if k == 0:
            return rnd.randrange(-10**6, 10**6)
        if k == 1:
            return rnd.choice([0, 2**63 - 1, -2**63, 2**64 + 7, -(10**30)])
        if k == 2:
            return rnd.choice([0.5, -1e-7, 1.5e300, 3.0, -2.25, 1e22, 1e16, 5e-324, -0.0, float("inf"), float("nan")])
        if k == 3:
            return rnd.choice([True, False, None])
        return _text(rnd, 12)
    if r < 0.6:
        seq = [_rand(rnd, depth + 1) for _ in range(rnd.randrange(0, 5))]
        return tuple(seq) if rnd.random() < 0.2 else seq
    return {_text(rnd, 6): _rand(rnd, depth + 1) for _ in range(rnd.randrange(0, 7))}


@pytest.mark.parametrize("seed", range(60))
def test_random_trees(seed):
    rnd = random.Random(seed)
    for _ in range(20):
        doc = _rand(rnd)
        assert oc.canonical(doc) == _want(doc)
        assert canonical_json(doc) == _want(doc)


def test_keys_sort_by_code_point():
    doc = {"b": 1, "a": 2, "B": 3, "": 4, "aa": 5, "é": 6, "z": 7, "中": 8, "\U0001F600": 9, "￿": 10, "a\x00": 11}
    assert oc.canonical(doc) == _want(doc)
    assert oc.canonical({"b": {"y": 1, "x": [{"q": 1, "p": 2}]}, "a": ()}) == b'{"a":[],"b":{"x":[{"p":2,"q":1}],"y":1}}'


def test_generated_pod_specs():
    for i, kw in enumerate(({}, {"gpus": 1}, {"gpus": 8, "annotations": {"amd.com/gpu-probe": "true"}},
                            {"image": "quay.io/opendatahub/workbench-images:jupyter-中文"})):
        nb = notebook(f"nb-{i}", "team-a", **kw)
        sts = generate_statefulset(nb, False, {})
        spec = sts["spec"]["template"]["spec"]
        for tree in (spec, defaults.pod_spec(deepcopy_json(spec)), sts["spec"]["template"], sts, nb):
            assert oc.canonical(tree) == _want(tree)
        tmpl = sts["spec"]["template"]
        import hashlib

        assert template_hash(sts) == f"{sts['metadata']['name']}-" + hashlib.sha1(
            _want(tmpl), usedforsecurity=False).hexdigest()[:10]
        # the cache of defaulted specs: one entry per content, whatever the member order
        reconcilehelper._DEFAULTED.clear()
        a = reconcilehelper._defaulted(spec)
        assert reconcilehelper._defaulted(dict(reversed(list(deepcopy_json(spec).items())))) is a
        assert list(reconcilehelper._DEFAULTED) == [_want(spec)]


class _Str(str):
    pass


@pytest.mark.parametrize("doc", [
    {1: "a", 2: "b"}, {"a": {None: 1}}, {True: 1}, {"a": _Str("x")}, {_Str("k"): 1}, {"a": 1.5, 3: 4},
    type("D", (dict,), {})({"b": 1, "a": 2}), {"a": type("L", (list,), {})([1, 2])},
], ids=["int-keys", "none-key", "bool-key", "str-subclass", "str-subclass-key", "mixed-keys", "dict-subclass",
        "list-subclass"])
def test_beyond_plain_trees_json_decides(doc):
    with pytest.raises(TypeError):
        oc.canonical(doc)
    try:
        want = _want(doc)
    except TypeError:  # keys json cannot order either
        with pytest.raises(TypeError):
            canonical_json(doc)
    else:
        assert canonical_json(doc) == want


def test_non_json_values_raise_as_json_does():
    for doc in ({"a": {1, 2}}, {"a": object()}, [b"x"]):
        with pytest.raises(TypeError):
            oc.canonical(doc)
        with pytest.raises(TypeError):
            canonical_json(doc)
    deep = cur = []
    for _ in range(600):
        cur.append([])
        cur = cur[0]
    with pytest.raises(ValueError):
        oc.canonical(deep)
