"""Informers whose watch events are applied where the bytes arrive (``runtime/informer.py``
``_StoreSink`` over the native ``WatchStore``, fed from ``http1._Conn.data_received``), against
the native and the Python apiserver, next to the Python path (``watch_batches`` without a
store) that stays as the fallback: subscribers must see the same thing either way."""

from __future__ import annotations

import asyncio

import pytest

pytest.importorskip("odh_kubeflow_amd.native._objcore")

from odh_kubeflow_amd.models import kinds  # noqa: E402
from odh_kubeflow_amd.models import meta as m  # noqa: E402
from odh_kubeflow_amd.runtime import informer as informer_mod  # noqa: E402
from odh_kubeflow_amd.runtime.informer import InformerCache  # noqa: E402
from odh_kubeflow_amd.runtime.rest import RestClient, RestConfig  # noqa: E402
from odh_kubeflow_amd.testing.apiserver.http import ApiServer  # noqa: E402
from odh_kubeflow_amd.testing.apiserver.store import ObjectStore  # noqa: E402


@pytest.fixture(params=["python", "native"])
def server_kind(request):
    return request.param


@pytest.fixture(params=["store", "python-path"])
def store_on(request, monkeypatch):
    if request.param != "store":
        monkeypatch.setattr(informer_mod, "_WatchStore", None)
    return request.param == "store"


class _Server:
    """An apiserver that can be stopped and started again on its port."""

    def __init__(self, kind: str, history: int = 4096):
        self.kind, self.history, self.port, self.srv = kind, history, 0, None
        self.store = ObjectStore()
        self.store.HISTORY = history

    async def start(self) -> "_Server":
        if self.kind == "native":
            from odh_kubeflow_amd.testing.apiserver.native import NativeApiServer

            self.srv = await NativeApiServer(history=self.history, port=self.port).start()
        else:
            self.srv = await ApiServer(self.store).start("127.0.0.1", self.port)
        self.port = self.srv.port
        return self

    async def stop(self) -> None:
        await self.srv.stop()

    def client(self) -> RestClient:
        return RestClient(RestConfig(host=self.srv.url))


async def _wait(pred, timeout=10.0):
    loop = asyncio.get_running_loop()
    end = loop.time() + timeout
    while loop.time() < end:
        if pred():
            return True
        await asyncio.sleep(0.005)
    return pred()


def _cm(name, ns, labels=None, data=None):
    return {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": name, "namespace": ns, "labels": labels or {}},
            "data": data or {}}


async def _namespaces(c, *names):
    for n in names:
        await c.create({"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": n}})


def _uses_store(cache, kind) -> bool:
    return cache.informer(kind)._sink is not None


def test_same_deliveries_under_concurrent_writers(run, server_kind, monkeypatch):
    """8 writers x 25 merge patches over 4 ConfigMaps: an informer fed through the native store
    and one on the Python path, watching side by side, make the same handler calls
    ``(type, name, resourceVersion, old's resourceVersion)`` in the same order."""
    async def go():
        srv = await _Server(server_kind).start()
        c, c_on, c_off = srv.client(), srv.client(), srv.client()
        caches = []
        try:
            await _namespaces(c, "a")
            for i in range(4):
                await c.create(_cm(f"cm{i}", "a"))
            seen = {}
            for name, rest in (("on", c_on), ("off", c_off)):
                if name == "off":
                    monkeypatch.setattr(informer_mod, "_WatchStore", None)
                cache = InformerCache(rest)
                caches.append(cache)
                calls = seen[name] = []
                cache.subscribe(kinds.CONFIG_MAP, lambda et, o, old, calls=calls: calls.append(
                    (et, m.name(o), m.resource_version(o), m.resource_version(old) if old else None)))
                await cache.wait_synced([kinds.CONFIG_MAP])
                assert _uses_store(cache, kinds.CONFIG_MAP) is (name == "on")
            written = []

            async def writer(t: int):
                for k in range(25):
                    out = await c.patch(kinds.CONFIG_MAP, {"data": {f"t{t}": str(k)}}, name=f"cm{(t * 3 + k) % 4}",
                                        namespace="a")
                    written.append(int(m.resource_version(out)))

            await asyncio.gather(*(writer(t) for t in range(8)))
            await c.delete(kinds.CONFIG_MAP, "cm3", "a")
            assert await _wait(lambda: all(len(s) == 4 + 200 + 1 for s in seen.values())), {k: len(v) for k, v in seen.items()}
            assert seen["on"] == seen["off"]
            mods = [int(rv) for et, _, rv, _ in seen["on"] if et == "MODIFIED"]
            assert mods == sorted(written) and seen["on"][-1][:2] == ("DELETED", "cm3")
            olds = {}  # every MODIFIED hands over the version the one before it brought
            for et, name, rv, old in seen["on"]:
                assert old == olds.get(name), (et, name, rv, old)
                olds[name] = rv
            on, off = (cache.informer(kinds.CONFIG_MAP) for cache in caches)
            assert on.items == off.items and (on.by_ns, on.rv, on.mutations) == (off.by_ns, off.rv, off.mutations)
        finally:
            for cache in caches:
                await cache.stop()
            for x in (c, c_on, c_off):
                await x.close()
            await srv.stop()
    run(go(), timeout=60)


def test_leaving_the_label_selector_is_a_delete(run, server_kind, store_on):
    async def go():
        srv = await _Server(server_kind).start()
        c = srv.client()
        cache = InformerCache(c, selectors={kinds.CONFIG_MAP: "sel=yes"})
        try:
            await _namespaces(c, "a")
            await c.create(_cm("in", "a", {"sel": "yes"}))
            await c.create(_cm("out", "a", {"sel": "no"}))
            seen = []
            cache.subscribe(kinds.CONFIG_MAP, lambda et, o, old: seen.append((et, m.name(o), old is not None)))
            await cache.wait_synced([kinds.CONFIG_MAP])
            assert _uses_store(cache, kinds.CONFIG_MAP) is store_on
            await c.patch(kinds.CONFIG_MAP, {"data": {"k": "v"}}, name="in", namespace="a")
            await c.patch(kinds.CONFIG_MAP, {"metadata": {"labels": {"sel": "no"}}}, name="in", namespace="a")
            await c.patch(kinds.CONFIG_MAP, {"metadata": {"labels": {"sel": "yes"}}}, name="out", namespace="a")
            assert await _wait(lambda: len(seen) >= 4)
            assert seen == [("ADDED", "in", False), ("MODIFIED", "in", True), ("DELETED", "in", True),
                            ("ADDED", "out", False)]
            inf = cache.informer(kinds.CONFIG_MAP)
            assert list(inf.items) == [("a", "out")] and inf.by_ns["a"] == {("a", "out")}
            assert cache.get(kinds.CONFIG_MAP, "in", "a") is None
        finally:
            await cache.stop()
            await c.close()
            await srv.stop()
    run(go(), timeout=60)


def test_namespace_filter_drops_fills_and_leaves_no_ghost(run, server_kind, store_on):
    """A cluster-wide informer behind a namespace filter: another namespace's events are dropped,
    a namespace that joins is listed once, and an object deleted while that list is in flight
    does not come back with it."""
    mine = {"a"}

    async def go():
        srv = await _Server(server_kind).start()
        c, other = srv.client(), srv.client()
        cache = InformerCache(c, namespace_filter=lambda o: m.name(o) in mine, cluster_watch=True)
        try:
            await _namespaces(other, "a", "b")
            await other.create(_cm("a1", "a"))
            for n in ("b1", "b2", "b3"):
                await other.create(_cm(n, "b"))
            seen = []
            cache.subscribe(kinds.CONFIG_MAP, lambda et, o, old: seen.append((et, m.name(o))))
            await cache.wait_synced([kinds.CONFIG_MAP, kinds.NAMESPACE])
            inf = cache.informer(kinds.CONFIG_MAP)
            assert (inf._sink is not None) is store_on and inf.ns_filter is not None
            await other.patch(kinds.CONFIG_MAP, {"data": {"k": "1"}}, name="b1", namespace="b")  # dropped
            await other.patch(kinds.CONFIG_MAP, {"data": {"k": "1"}}, name="a1", namespace="a")
            assert await _wait(lambda: ("MODIFIED", "a1") in seen)
            assert seen == [("ADDED", "a1"), ("MODIFIED", "a1")] and list(inf.items) == [("a", "a1")]
            # "b" joins; its list is held back while b2 is deleted and b3 modified
            real_list, gate = c.list_rv, asyncio.get_running_loop().create_future()
            listing = asyncio.Event()

            async def held_list(kind, namespace=None, *a, **kw):
                out = await real_list(kind, namespace, *a, **kw)
                if namespace == "b":
                    listing.set()
                    await gate
                return out

            c.list_rv = held_list
            mine.add("b")
            cache.refresh_namespace("b")
            await asyncio.wait_for(listing.wait(), 10)
            await other.delete(kinds.CONFIG_MAP, "b2", "b")
            await other.patch(kinds.CONFIG_MAP, {"data": {"k": "2"}}, name="b3", namespace="b")
            assert await _wait(lambda: ("DELETED", "b2") in seen and ("b", "b3") in inf.items)
            gate.set_result(None)
            assert await _wait(lambda: ("b", "b1") in inf.items and not inf._fill_tombstones)
            c.list_rv = real_list
            assert sorted(inf.items) == [("a", "a1"), ("b", "b1"), ("b", "b3")]  # no ghost of b2
            assert inf.items[("b", "b3")]["data"] == {"k": "2"} and ("ADDED", "b2") not in seen
            assert inf.by_ns["b"] == {("b", "b1"), ("b", "b3")}
            # "b" leaves again: to the subscribers its objects are gone
            mine.discard("b")
            cache.refresh_namespace("b")
            assert await _wait(lambda: sorted(inf.items) == [("a", "a1")])
            assert {("DELETED", "b1"), ("DELETED", "b3")} <= set(seen[-2:])
        finally:
            await cache.stop()
            await c.close()
            await other.close()
            await srv.stop()
    run(go(), timeout=60)


def test_handler_exception_does_not_stop_later_events(run, server_kind, store_on):
    async def go():
        srv = await _Server(server_kind).start()
        c = srv.client()
        cache = InformerCache(c)
        try:
            await _namespaces(c, "a")
            seen = []

            def handler(et, o, old):
                seen.append((et, m.name(o)))
                if m.name(o) == "bad":
                    raise RuntimeError("handler bug")

            cache.subscribe(kinds.CONFIG_MAP, handler)
            cache.subscribe(kinds.CONFIG_MAP, lambda et, o, old: seen.append(("second", m.name(o))))
            await cache.wait_synced([kinds.CONFIG_MAP])
            watches = c.by_verb.get("WATCH", 0)
            await c.create(_cm("bad", "a"))
            await c.create(_cm("good", "a"))
            assert await _wait(lambda: ("second", "good") in seen)
            assert seen == [("ADDED", "bad"), ("second", "bad"), ("ADDED", "good"), ("second", "good")]
            assert c.by_verb.get("WATCH", 0) == watches  # the stream was not failed by it
        finally:
            await cache.stop()
            await c.close()
            await srv.stop()
    run(go(), timeout=60)


def test_watch_timeout_resumes_from_the_last_version(run, server_kind, store_on):
    """A watch the server closes at its timeout (one second here, the shortest there is) is
    reopened from the last resourceVersion seen: no relist, nothing delivered twice, nothing missed."""
    async def go():
        srv = await _Server(server_kind).start()
        c, other = srv.client(), srv.client()
        cache = InformerCache(c, namespace="a", watch_timeout_s=1)
        try:
            await _namespaces(other, "a")
            await other.create(_cm("x", "a"))
            seen = []
            cache.subscribe(kinds.CONFIG_MAP, lambda et, o, old: seen.append((et, m.name(o), (o.get("data") or {}).get("k"))))
            await cache.wait_synced([kinds.CONFIG_MAP])
            inf = cache.informer(kinds.CONFIG_MAP)
            assert (inf._sink is not None) is store_on
            await other.patch(kinds.CONFIG_MAP, {"data": {"k": "1"}}, name="x", namespace="a")
            assert await _wait(lambda: len(seen) == 2)
            watches = c.by_verb["WATCH"]
            assert await _wait(lambda: c.by_verb["WATCH"] > watches, 10)  # timed out and reopened
            await other.patch(kinds.CONFIG_MAP, {"data": {"k": "2"}}, name="x", namespace="a")
            assert await _wait(lambda: len(seen) == 3)
            assert seen == [("ADDED", "x", None), ("MODIFIED", "x", "1"), ("MODIFIED", "x", "2")] and inf.relists == 1
        finally:
            await cache.stop()
            await c.close()
            await other.close()
            await srv.stop()
    run(go(), timeout=60)


def test_server_restart_and_gone_lead_to_a_relist(run, server_kind, store_on):
    """The informer's stream is lost and it reconnects from a resourceVersion the server no longer
    has: a history of 8, rolled over by writes the informer does not watch.  It is answered 410,
    relists, raises events for the difference and ends up with what the server holds.  The
    Python apiserver is stopped and started again on its port, with its objects; a new native
    process would come back empty, its versions below the informer's, so there the watch
    connection is cut instead."""
    async def go():
        srv = await _Server(server_kind, history=8).start()
        c, other = srv.client(), srv.client()
        cache = InformerCache(c, namespace="a")
        try:
            conns = []
            pool, connect = c._http(), c._http()._connect

            async def recording_connect():
                conns.append(await connect())
                return conns[-1]

            pool._connect = recording_connect
            await _namespaces(other, "a", "elsewhere")
            await other.create(_cm("before", "a"))
            await other.create(_cm("doomed", "a"))
            seen = []
            cache.subscribe(kinds.CONFIG_MAP, lambda et, o, old: seen.append((et, m.name(o))))
            await cache.wait_synced([kinds.CONFIG_MAP])
            inf = cache.informer(kinds.CONFIG_MAP)
            assert (inf._sink is not None) is store_on and inf.relists == 1
            assert await _wait(lambda: any(x._streaming and x._head is not None for x in conns))
            live = [x for x in conns if x._streaming and not x.closed]
            assert len(live) == 1 and live[0]._sink_on is store_on
            for i in range(12):  # not this informer's namespace: its resourceVersion stays behind
                await other.create(_cm(f"e{i}", "elsewhere"))
            watches = c.by_verb["WATCH"]
            if server_kind == "python":
                await srv.stop()
                await other.close()
                await srv.start()
                other = srv.client()
            else:
                live[0].transport.abort()
            # what happens while the informer is away shows as the relist's difference
            await other.delete(kinds.CONFIG_MAP, "doomed", "a")
            await other.create(_cm("after", "a"))
            assert await _wait(lambda: ("ADDED", "after") in seen and ("DELETED", "doomed") in seen, 15)
            assert c.by_verb["WATCH"] > watches and inf.relists == 2
            assert seen[:2] == [("ADDED", "before"), ("ADDED", "doomed")]
            assert sorted(seen[2:]) == [("ADDED", "after"), ("DELETED", "doomed")]  # each once, whichever way it came
            assert set(inf.items) == {("a", "before"), ("a", "after")} == inf.by_ns["a"]
            # and the new stream delivers
            await other.patch(kinds.CONFIG_MAP, {"data": {"k": "1"}}, name="after", namespace="a")
            assert await _wait(lambda: seen[-1] == ("MODIFIED", "after"))
        finally:
            await cache.stop()
            await c.close()
            await other.close()
            await srv.stop()
    run(go(), timeout=60)
