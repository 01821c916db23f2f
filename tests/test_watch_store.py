"""The native watch store (``native/objcore.cpp`` ``WatchStore``, framing in
``native/watch_feed.hpp``) against the Python path it replaces.

The reference is that path itself, kept as the fallback: ``http1._dechunk``, the split into
lines, ``loads_event`` with a lookup into the store, and ``_Informer._transform`` / ``_put`` /
``_delete``.  One recorded watch response of about 40 events (Notebook-, Pod- and Event-sized
objects added, modified and deleted, a BOOKMARK, non-ASCII text, ``\\u`` escapes with a
surrogate pair, an integer of more than 18 digits, a float, a blank keep-alive line, a chunk
extension, two events in one chunk, one event over three chunks, the terminal chunk with a
trailer) is fed whole, byte by byte, cut in two at every offset and cut in five at 500 seeded
random places: every feeding must give the reference's deltas and the reference's final dict.
"""

from __future__ import annotations

import json
import random

import pytest

oc = pytest.importorskip("odh_kubeflow_amd.native._objcore")

from odh_kubeflow_amd.models.errors import ApiError, Gone  # noqa: E402
from odh_kubeflow_amd.models.scheme import SCHEME  # noqa: E402
from odh_kubeflow_amd.runtime import informer as informer_mod  # noqa: E402
from odh_kubeflow_amd.runtime.http1 import _dechunk  # noqa: E402
from odh_kubeflow_amd.runtime.informer import InformerCache, _Informer  # noqa: E402

NS = "team-a"
BIG = 123456789012345678901234  # more than 18 digits: beyond the decoder's fast path


def _managed(n=2):
    return [{"manager": f"m{i}", "operation": "Update", "apiVersion": "v1", "time": "2024-01-01T00:00:00Z",
             "fieldsType": "FieldsV1", "fieldsV1": {"f:metadata": {"f:labels": {".": {}, "f:app": {}}},
                                                    "f:spec": {"f:template": {"f:spec": {"f:containers": {}}}}}}
            for i in range(n)]


def _notebook(name, rv, status=None, labels=None):
    o = {"apiVersion": "kubeflow.org/v1", "kind": "Notebook",
         "metadata": {"name": name, "namespace": NS, "uid": f"uid-{name}", "resourceVersion": str(rv),
                      "generation": 1, "creationTimestamp": "2024-01-01T00:00:00Z",
                      "labels": labels or {"app": name, "opendatahub.io/dashboard": "true"},
                      "annotations": {"notebooks.opendatahub.io/inject-oauth": "true",
                                      "openshift.io/display-name": "Tëst nötebook 中文 \U0001F600",
                                      "openshift.io/description": 'quote " backslash \\ tab \t done'},
                      "managedFields": _managed(2)},
         "spec": {"template": {"spec": {"containers": [{
             "name": name, "image": "quay.io/opendatahub/workbench-images:jupyter-rocm-pytorch",
             "resources": {"limits": {"amd.com/gpu": "1", "cpu": "2", "memory": "8Gi"},
                           "requests": {"cpu": "500m", "memory": "4Gi"}},
             "env": [{"name": "NOTEBOOK_ARGS", "value": "--ServerApp.port=8888"}, {"name": "JUPYTER_IMAGE", "value": "x"}],
             "ports": [{"containerPort": 8888, "name": "notebook-port", "protocol": "TCP"}],
             "volumeMounts": [{"mountPath": "/opt/app-root/src", "name": name}]}],
             "volumes": [{"name": name, "persistentVolumeClaim": {"claimName": name}}]}}}}
    if status is not None:
        o["status"] = status
    return o


def _pod(name, rv, phase="Pending", owner="uid-nb-0", labels=None):
    return {"metadata": {"name": name, "namespace": NS, "uid": f"uid-{name}", "resourceVersion": str(rv),
                         "labels": labels if labels is not None else {"notebook-name": "nb-0", "statefulset": "nb-0"},
                         "ownerReferences": [{"apiVersion": "apps/v1", "kind": "StatefulSet", "name": "nb-0",
                                              "uid": owner, "controller": True}],
                         "managedFields": _managed(3)},
            "spec": {"nodeName": "node-0", "schedulerName": "default-scheduler", "priority": 0,
                     "terminationGracePeriodSeconds": 30,
                     "containers": [{"name": "nb", "image": "img:1", "resources": {"limits": {"amd.com/gpu": "1"}},
                                     "ports": [{"containerPort": 8888}]},
                                    {"name": "oauth-proxy", "image": "proxy:2", "args": ["--https-address=:8443"]}]},
            "status": {"phase": phase, "startTime": "2024-01-01T00:00:00Z", "load": 0.25, "observed": BIG,
                       "conditions": [{"type": "Ready", "status": "True" if phase == "Running" else "False"}]}}


def _event(i, rv, count=1):
    return {"metadata": {"name": f"nb-0.{i:04x}", "namespace": NS, "resourceVersion": str(rv), "uid": f"uid-ev-{i}"},
            "involvedObject": {"kind": "Pod", "name": "nb-0-0", "namespace": NS, "uid": "uid-nb-0-0"},
            "reason": "Pulled", "message": f"Successfully pulled image “img:{i}” in {i}.5s", "type": "Normal",
            "count": count, "firstTimestamp": "2024-01-01T00:00:00Z", "lastTimestamp": "2024-01-01T00:00:01Z"}


def _line(etype, obj, **kw) -> bytes:
    return json.dumps({"type": etype, "object": obj}, separators=(",", ":"), **kw).encode() + b"\n"


def _chunk(data: bytes, ext: bytes = b"") -> bytes:
    return b"%x%s\r\n%s\r\n" % (len(data), ext, data)


def _events():
    """(type, object) of the recorded stream, in order."""
    rv = iter(range(100, 1000))
    ready = {"readyReplicas": 1, "conditions": [{"type": "Ready", "status": "True"}], "containerState": {"running": {}}}
    ev = [("ADDED", _notebook("nb-0", next(rv))), ("ADDED", _notebook("nb-1", next(rv))),
          ("ADDED", _pod("nb-0-0", next(rv))),
          ("MODIFIED", _notebook("nb-0", next(rv), status={"readyReplicas": 0})),
          ("MODIFIED", _pod("nb-0-0", next(rv), "Running")),
          ("MODIFIED", _notebook("nb-0", next(rv), status=ready)),
          ("ADDED", _pod("nb-1-0", next(rv), owner="uid-nb-1", labels={"notebook-name": "nb-1"})),
          ("BOOKMARK", {"kind": "Pod", "apiVersion": "v1", "metadata": {"resourceVersion": str(next(rv))}})]
    for i in range(24):
        ev.append(("ADDED", _event(i, next(rv))))
        if i % 6 == 5:
            ev.append(("MODIFIED", _event(i, next(rv), count=2)))
    ev += [("MODIFIED", _pod("nb-1-0", next(rv), "Running", owner="uid-nb-1", labels={})),
           ("DELETED", _event(3, next(rv))), ("DELETED", _pod("nb-0-0", next(rv), "Running")),
           ("DELETED", _notebook("nb-1", next(rv))), ("DELETED", _event(999, next(rv)))]  # the last: never stored
    return ev


def _stream() -> bytes:
    ev = _events()
    lines = [_line(t, o) for t, o in ev]
    # \u escapes (json's default) with a surrogate pair for the first notebook, raw UTF-8 for the rest
    lines[1] = _line(*ev[1], ensure_ascii=False)
    lines[3] = _line(*ev[3], ensure_ascii=False)
    assert b"\\ud83d\\ude00" in lines[0] and "\U0001F600".encode() in lines[1]
    out = [_chunk(lines[0], b";ext=1;other=\"a b\""),
           _chunk(lines[1] + lines[2]),  # two events in one chunk
           _chunk(b"\n"),  # a blank keep-alive line
           _chunk(lines[3][:100]), _chunk(lines[3][100:700]), _chunk(lines[3][700:])]  # one event over three chunks
    out += [_chunk(x) for x in lines[4:]]
    out.append(b"0\r\nX-Trailer: done\r\n\r\n")
    return b"".join(out)


STREAM = _stream()
N_EVENTS = len(_events())


def _new_informer(native: bool, kind="v1/Pod", **cache_kw) -> _Informer:
    info = SCHEME.resolve(kind)
    saved = informer_mod._WatchStore
    if not native:
        informer_mod._WatchStore = None
    try:
        inf = _Informer(InformerCache(None, **cache_kw), info, info.storage_version)
    finally:
        informer_mod._WatchStore = saved
    assert (inf._sink is not None) == native
    return inf


def _reference(pieces):
    """Today's path over ``pieces`` of the response body: the deltas and the informer."""
    inf = _new_informer(False)
    raw, body, deltas = bytearray(), bytearray(), []
    for piece in pieces:
        raw += piece
        _dechunk(raw, body)
        *lines, rest = bytes(body).split(b"\n")
        body[:] = rest
        for line in lines:
            if not line or line.isspace():
                continue
            try:
                et, obj = oc.loads_event(line, inf._stored)
            except ValueError:
                ev = json.loads(line)
                et, obj = ev.get("type"), ev.get("object") or {}
            if et == "BOOKMARK":
                deltas.append((et, obj, None))
                continue
            obj = inf._transform(obj)
            deltas.append((et, obj, inf._delete(obj) if et == "DELETED" else inf._put(obj)))
    return deltas, inf


@pytest.fixture(scope="module")
def expected():
    deltas, inf = _reference([STREAM])
    assert len(deltas) == N_EVENTS and 38 <= N_EVENTS <= 44
    return deltas, dict(inf.items)


def _feed(pieces, apply=True):
    st = oc.WatchStore("v1", "Pod")
    st.begin(-2)
    deltas = []
    for p in pieces:
        deltas += st.feed(p, apply)
    return deltas, st


def _splits(cuts):
    cuts = [0, *sorted(cuts), len(STREAM)]
    return [STREAM[a:b] for a, b in zip(cuts, cuts[1:])]


def test_whole(expected):
    deltas, st = _feed([STREAM])
    assert deltas == expected[0]
    assert st.items == expected[1] and type(st.items) is dict
    assert st.done and st.failed is None
    assert [json.dumps(d[1]) for d in deltas] == [json.dumps(d[1]) for d in expected[0]]  # member order too


def test_byte_by_byte(expected):
    deltas, st = _feed([STREAM[i:i + 1] for i in range(len(STREAM))])
    assert deltas == expected[0] and st.items == expected[1] and st.done


def test_cut_in_two_at_every_offset(expected):
    want_deltas, want_items = expected
    for i in range(len(STREAM) + 1):
        deltas, st = _feed([STREAM[:i], STREAM[i:]])
        assert deltas == want_deltas and st.items == want_items and st.done, i


def test_cut_in_five_at_random(expected):
    rnd = random.Random(20240)
    for _ in range(500):
        cuts = [rnd.randrange(len(STREAM) + 1) for _ in range(4)]
        deltas, st = _feed(_splits(cuts))
        assert deltas == expected[0] and st.items == expected[1] and st.done, cuts


def test_without_apply_the_dict_is_the_callers(expected):
    """``apply=False``: the same objects, decoded against whatever the caller has stored."""
    deltas, st = _feed([STREAM], apply=False)
    assert [(t, o) for t, o, _ in deltas] == [(t, o) for t, o, _ in expected[0]]
    assert all(old is None for _, _, old in deltas) and st.items == {}


def test_informer_deliveries_match(expected):
    """Through ``_StoreSink`` the subscribers see what ``_apply`` shows them, and the indexes agree."""
    def record(inf):
        seen = []
        inf.handlers = {0: (None, lambda et, obj, old: seen.append((et, obj, old)))}
        return seen

    ref = _new_informer(False)
    want = record(ref)
    for et, obj, _ in _reference([STREAM])[0]:
        ref._apply(et, json.loads(json.dumps(obj)))
    rnd = random.Random(7)
    for cuts in ([], [rnd.randrange(len(STREAM)) for _ in range(4)]):
        inf = _new_informer(True)
        got = record(inf)
        assert inf._sink.begin(-2) is False
        ended = [inf._sink.data(p) for p in _splits(cuts)]
        assert ended[-1] is True
        assert got == want and len(got) == N_EVENTS - 1  # all but the BOOKMARK
        assert inf.items == ref.items and inf.items is inf._sink.store.items
        assert (inf.by_ns, inf.by_owner, inf.by_label) == (ref.by_ns, ref.by_owner, ref.by_label)
        assert inf.rv == ref.rv and inf.mutations == ref.mutations and inf.events == ref.events


def test_unchanged_subtrees_are_the_stored_ones():
    deltas, _ = _feed([STREAM])
    status_only = [(new, old) for t, new, old in deltas
                   if t == "MODIFIED" and old is not None and new.get("kind") == "Notebook"]
    assert len(status_only) == 2
    for new, old in status_only:
        assert new["spec"] is old["spec"] and new["metadata"] is not old["metadata"]
        assert new["metadata"]["labels"] is old["metadata"]["labels"]


def test_managed_fields_are_never_built():
    deltas, st = _feed([STREAM])
    assert b"managedFields" in STREAM
    for _, new, old in deltas:
        assert "managedFields" not in new["metadata"]
    assert all("managedFields" not in o["metadata"] for o in st.items.values())
    # only the event object's own metadata.managedFields is dropped
    line = _line("ADDED", {"metadata": {"name": "x", "managedFields": [1]}, "managedFields": 1,
                           "spec": {"managedFields": 2, "metadata": {"managedFields": 3}},
                           "list": [{"managedFields": 4}]})
    (_, obj, _), = _feed([_chunk(line)])[0]
    assert obj == {"metadata": {"name": "x"}, "managedFields": 1, "apiVersion": "v1", "kind": "Pod",
                   "spec": {"managedFields": 2, "metadata": {"managedFields": 3}}, "list": [{"managedFields": 4}]}


@pytest.mark.parametrize("code,exc", [(410, Gone), (500, ApiError)])
def test_error_event_mid_batch(code, exc):
    status = {"kind": "Status", "apiVersion": "v1", "status": "Failure", "code": code, "reason": "Expired",
              "message": "too old resource version"}
    body = _chunk(_line("ADDED", _pod("a", 1)) + _line("ADDED", _pod("b", 2)) + _line("ERROR", status)
                  + _line("ADDED", _pod("c", 3)))
    deltas, st = _feed([body])
    assert [d[0] for d in deltas] == ["ADDED", "ADDED", "ERROR"] and deltas[-1][1:] == (status, None)
    assert sorted(st.items) == [(NS, "a"), (NS, "b")] and st.done
    inf = _new_informer(True)
    seen = []
    inf.handlers = {0: (None, lambda et, obj, old: seen.append((et, obj["metadata"]["name"])))}
    inf._sink.begin(-2)
    with pytest.raises(exc) as e:
        inf._sink.data(body)
    assert type(e.value) is exc or exc is ApiError
    assert seen == [("ADDED", "a"), ("ADDED", "b")] and sorted(inf.items) == [(NS, "a"), (NS, "b")]


def test_nan_line_goes_to_json_and_the_stream_goes_on():
    nan = b'{"type":"ADDED","object":{"metadata":{"name":"n","namespace":"team-a","resourceVersion":"7"},"v":NaN}}\n'
    body = _chunk(_line("ADDED", _pod("a", 1)) + nan + _line("ADDED", _pod("b", 9)))
    deltas, st = _feed([body])
    assert [d[0] for d in deltas] == ["ADDED", None, "ADDED"] and deltas[1] == (None, nan[:-1], None)
    assert sorted(st.items) == [(NS, "a"), (NS, "b")]
    inf = _new_informer(True)
    inf._sink.begin(-2)
    inf._sink.data(body)
    assert sorted(inf.items) == [(NS, "a"), (NS, "b"), (NS, "n")] and inf.items[(NS, "n")]["v"] != inf.items[(NS, "n")]["v"]
    assert inf.items[(NS, "n")]["kind"] == "Pod" and inf.rv == "9"


DEEP = b'{"type":"ADDED","object":{"metadata":{"name":"deep"},"v":' + b"[" * 600 + b"]" * 600 + b"}}\n"


@pytest.mark.parametrize("bad", [
    b"zz\r\n{}\n\r\n",  # a chunk size that is no hex number
    b"\r\n",  # an empty chunk size
    b"1" * 17 + b"\r\n",  # an oversized one
    b"-5\r\nabcde\r\n",
    _chunk(_line("ADDED", _pod("x", 5)))[:-2] + b"XY",  # no CRLF after the chunk data
    _chunk(_line("ADDED", _pod("x", 5)))[:-1] + b"Y",
    _chunk(DEEP),  # JSON nested deeper than 512
], ids=["size-not-hex", "size-empty", "size-oversized", "size-negative", "no-crlf", "no-lf", "too-deep"])
def test_malformed_input_raises_and_leaves_the_store_whole(bad):
    good = _chunk(_line("ADDED", _pod("a", 1)))
    # nothing before the fault in the call: raised at once
    st = oc.WatchStore("v1", "Pod")
    st.begin(-2)
    assert len(st.feed(good)) == 1
    before = dict(st.items)
    if b"\"x\"" in bad:  # the event of the faulty chunk is complete: handed over, then the fault
        assert [d[1]["metadata"]["name"] for d in st.feed(bad)] == ["x"]
        before = dict(st.items)
        assert (NS, "x") in before
    with pytest.raises(ValueError):
        st.feed(bad if b"\"x\"" not in bad else b"")
    assert st.failed and st.items == before
    with pytest.raises(ValueError):  # and it stays failed until the next body begins
        st.feed(good)
    assert st.items == before
    # events before the fault in the same call are handed over first, and are in the dict
    st = oc.WatchStore("v1", "Pod")
    st.begin(-2)
    deltas = st.feed(good + bad)
    assert deltas[0][1]["metadata"]["name"] == "a" and (NS, "a") in st.items and st.failed
    with pytest.raises(ValueError):
        st.feed(b"")
    assert len(st.items) == len(deltas)
    st.begin(-2)  # a new body: readable again, the objects kept
    assert st.failed is None and len(st.feed(_chunk(_line("ADDED", _pod("b", 2))))) == 1
    # through the sink: the stream fails with ValueError after the deliveries
    inf = _new_informer(True)
    inf._sink.begin(-2)
    with pytest.raises(ValueError):
        inf._sink.data(good + bad)
    assert (NS, "a") in inf.items and inf.by_ns[NS] == set(inf.items)


def test_length_and_eof_delimited_bodies():
    lines = _line("ADDED", _pod("a", 1)) + b"\r\n" + _line("MODIFIED", _pod("a", 2, "Running"))
    for want in (len(lines), -3):
        for cut in range(len(lines) + 1):
            st = oc.WatchStore("v1", "Pod")
            st.begin(want)
            deltas = st.feed(lines[:cut]) + st.feed(lines[cut:] + (b"next response" if want >= 0 else b""))
            assert [d[0] for d in deltas] == ["ADDED", "MODIFIED"] and deltas[1][2] is deltas[0][1]
            assert st.done is (want >= 0)
