"""Watch delivery of the native apiserver: events are carried to the watchers by the thread that
committed them, each object version serialised once.

What must hold whichever thread carries an event: every watcher gets its resource's events in
resourceVersion order, none missing and none twice, under concurrent writers; a watcher that
does not read (or vanishes) never holds a write up; the bytes of a watch event's object are the
write's response body; and what rides along — the admission webhook cache, the request
accounting — shows a change at once.  The watchers here read the wire themselves (raw sockets,
chunked encoding), so a torn or doubled chunk would not be smoothed over by a client library."""

import asyncio
import json
import socket
import struct

import pytest

from odh_kubeflow_amd.models import kinds
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.runtime.rest import RestClient, RestConfig
from odh_kubeflow_amd.testing.apiserver import native

pytestmark = pytest.mark.skipif(not native.available(), reason="native apiserver not built")

CM = "/api/v1/namespaces/{ns}/configmaps"


class RawWatch:
    """One watch stream read off a socket: ``events`` are ``(type, object)`` in arrival order.
    Every chunk must be whole lines, every line one JSON document (asserted as they arrive)."""

    def __init__(self, port: int, target: str, rcvbuf: int = 0):
        self.port, self.target, self.rcvbuf = port, target, rcvbuf
        self.events = []
        self.ended = False  # the terminating chunk or EOF
        self.reader = self.writer = self.sock = None

    async def open(self) -> "RawWatch":
        self.sock = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        if self.rcvbuf:
            self.sock.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, self.rcvbuf)
        self.sock.setblocking(False)
        await asyncio.get_running_loop().sock_connect(self.sock, ("127.0.0.1", self.port))
        kw = {"limit": self.rcvbuf} if self.rcvbuf else {}
        self.reader, self.writer = await asyncio.open_connection(sock=self.sock, **kw)
        self.writer.write(f"GET {self.target} HTTP/1.1\r\nHost: x\r\n\r\n".encode())
        await self.writer.drain()
        return self

    async def head(self) -> None:
        status = await self.reader.readline()
        assert status.startswith(b"HTTP/1.1 200"), status
        while (await self.reader.readline()) not in (b"\r\n", b""):
            pass

    async def read_until(self, done) -> None:
        """Read chunks until ``done(self)`` or the stream ends."""
        while not done(self) and not self.ended:
            size_line = await self.reader.readline()
            if not size_line:
                self.ended = True
                return
            n = int(size_line.strip(), 16)
            if n == 0:
                self.ended = True
                return
            data = await self.reader.readexactly(n)
            assert await self.reader.readexactly(2) == b"\r\n"
            assert data.endswith(b"\n"), data[-40:]
            for line in data[:-1].split(b"\n"):
                ev = json.loads(line)  # exactly one document per line
                assert set(ev) == {"type", "object"}, list(ev)
                self.events.append((ev["type"], ev["object"]))

    def abort(self) -> None:
        """Close with a reset, unread data and all."""
        self.sock.setsockopt(socket.SOL_SOCKET, socket.SO_LINGER, struct.pack("ii", 1, 0))
        self.writer.transport.abort()

    def close(self) -> None:
        if self.writer is not None:
            self.writer.transport.abort()


def rv_of(obj) -> int:
    return int(obj["metadata"]["resourceVersion"])


def keys(events):
    return [(o["metadata"]["name"], rv_of(o)) for _t, o in events]


def assert_ordered(events):
    rvs = [rv_of(o) for t, o in events if t != "ERROR"]
    assert all(a < b for a, b in zip(rvs, rvs[1:])), "resourceVersions out of order or repeated"


async def start():
    nat = await native.NativeApiServer().start()
    return nat, RestClient(RestConfig(host=nat.url))


async def namespace(c, *names):
    for n in names:
        await c.create({"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": n}})


def configmap(name, ns, labels=None, data=None):
    return {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": name, "namespace": ns, "labels": labels or {}},
            "data": data or {}}


def test_order_under_concurrent_writers(run):
    """8 writers x 40 merge patches over 4 ConfigMaps in each of two namespaces; a namespace-
    scoped, a cluster-wide and a label-selected watcher each see exactly the writes they want,
    in resourceVersion order."""
    async def go():
        nat, c = await start()
        watches = []
        try:
            await namespace(c, "a", "b")
            for ns in ("a", "b"):
                for i in range(4):
                    await c.create(configmap(f"cm{i}", ns, {"sel": "yes" if i % 2 else "no"}))
            _, rv0 = await c.list_rv(kinds.CONFIG_MAP)
            q = f"?watch=true&resourceVersion={rv0}&timeoutSeconds=60"
            watches = [await RawWatch(nat.port, CM.format(ns="a") + q).open(),
                       await RawWatch(nat.port, "/api/v1/configmaps" + q).open(),
                       await RawWatch(nat.port, "/api/v1/configmaps" + q + "&labelSelector=sel%3Dyes").open()]
            for w in watches:
                await w.head()
            written = []  # (namespace, name, resourceVersion) of every write response

            async def writer(t: int):
                for k in range(40):
                    ns, name = ("a", "b")[(t + k) % 2], f"cm{(t * 7 + k) % 4}"
                    out = await c.patch(kinds.CONFIG_MAP, {"data": {f"t{t}": str(k)}}, name=name, namespace=ns)
                    written.append((ns, name, rv_of(out)))

            await asyncio.gather(*(writer(t) for t in range(8)))
            assert len(written) == 320 and len({rv for _, _, rv in written}) == 320
            want = [{(n, rv) for ns, n, rv in written if ns == "a"},
                    {(n, rv) for _, n, rv in written},
                    {(n, rv) for _, n, rv in written if n in ("cm1", "cm3")}]
            for w, exp in zip(watches, want):
                await asyncio.wait_for(w.read_until(lambda w, n=len(exp): len(w.events) >= n), 20)
                assert {t for t, _ in w.events} == {"MODIFIED"}
                assert_ordered(w.events)
                got = keys(w.events)
                assert len(got) == len(set(got)), "an event was delivered twice"
                assert set(got) == exp
            prof = (await nat.stats())["prof"]
            assert prof["watch_direct"] + prof["watch_fallback"] > 0
        finally:
            for w in watches:
                w.close()
            await c.close()
            await nat.stop()
    run(go(), timeout=60)


def test_slow_consumer_never_blocks_a_commit(run):
    """A watcher that stops reading: 200 creates of 16 KiB ConfigMaps all complete meanwhile.
    Reading again it gets every event in order, or an in-order prefix and then 410 / the end
    of the stream — never a gap or a reorder.  A healthy watcher next to it sees all 200."""
    async def go():
        nat, c = await start()
        slow = healthy = None
        try:
            await namespace(c, "s")
            _, rv0 = await c.list_rv(kinds.CONFIG_MAP)
            q = f"?watch=true&resourceVersion={rv0}&timeoutSeconds=60"
            slow = await RawWatch(nat.port, CM.format(ns="s") + q, rcvbuf=4096).open()
            healthy = await RawWatch(nat.port, CM.format(ns="s") + q).open()
            await healthy.head()
            reading = asyncio.ensure_future(healthy.read_until(lambda w: len(w.events) >= 200))
            blob = "x" * (16 << 10)
            created = []
            for i in range(200):  # `slow` is not being read
                created.append(rv_of(await c.create(configmap(f"big{i}", "s", data={"blob": blob}))))
            await reading
            assert [rv_of(o) for _, o in healthy.events] == created
            print("prof after the creates:", {k: v for k, v in (await nat.stats())["prof"].items() if k.startswith("watch_")})
            await slow.head()
            await slow.read_until(lambda w: len(w.events) >= 200 or (w.events and w.events[-1][0] == "ERROR"))
            evs = slow.events
            if evs and evs[-1][0] == "ERROR":
                assert evs[-1][1]["code"] == 410
                evs = evs[:-1]
            assert [rv_of(o) for _, o in evs] == created[:len(evs)], "a gap or a reorder"
            assert len(evs) == 200 or slow.ended or slow.events[-1][0] == "ERROR"
        finally:
            for w in (slow, healthy):
                if w is not None:
                    w.close()
            await c.close()
            await nat.stop()
    run(go(), timeout=30)  # a hang guard, not a measurement


def test_watcher_vanishes_mid_burst(run):
    """The watch socket is reset while writers run: the writes go on, /healthz answers, a new
    watch from the last resourceVersion seen gets the remainder, and the slot is released."""
    import aiohttp

    async def go():
        nat, c = await start()
        w = w2 = None
        try:
            await namespace(c, "v")
            _, rv0 = await c.list_rv(kinds.CONFIG_MAP)
            assert (await nat.stats())["prof"]["watch_slots"] == 0
            w = await RawWatch(nat.port, CM.format(ns="v") + f"?watch=true&resourceVersion={rv0}&timeoutSeconds=60").open()
            await w.head()
            written = []

            async def writer(t: int):
                for k in range(50):
                    written.append(rv_of(await c.create(configmap(f"w{t}-{k}", "v", data={"k": "v" * 512}))))

            writers = asyncio.gather(*(writer(t) for t in range(4)))
            await w.read_until(lambda w: len(w.events) >= 20)
            assert (await nat.stats())["prof"]["watch_slots"] == 1
            w.abort()  # mid-burst
            await writers
            assert_ordered(w.events)
            last = rv_of(w.events[-1][1])
            async with aiohttp.ClientSession() as s:
                async with s.get(nat.url + "/healthz") as r:
                    assert r.status == 200 and await r.text() == "ok"
            w2 = await RawWatch(nat.port, CM.format(ns="v") + f"?watch=true&resourceVersion={last}&timeoutSeconds=60").open()
            await w2.head()
            rest = sorted(rv for rv in written if rv > last)
            await asyncio.wait_for(w2.read_until(lambda w: len(w.events) >= len(rest)), 10)
            assert [rv_of(o) for _, o in w2.events] == rest
            w2.close()
            # both streams are gone: a write finds the dead socket (or the stream's own check does)
            slots = None
            for i in range(400):
                await c.create(configmap(f"after{i}", "v"))
                slots = (await nat.stats())["prof"]["watch_slots"]
                if slots == 0:
                    break
                await asyncio.sleep(0.02)
            assert slots == 0
        finally:
            for x in (w, w2):
                if x is not None:
                    x.close()
            await c.close()
            await nat.stop()
    run(go(), timeout=60)


def test_one_serialisation_same_bytes(run):
    """The object of a watch event is the write's response body (as parsed JSON), in the version
    the watcher asked for; a dry-run create and a no-op patch emit nothing and leave the
    resourceVersion where it was."""
    import aiohttp

    async def go():
        nat, c = await start()
        watches = []
        try:
            await namespace(c, "o")
            _, rv0 = await c.list_rv(kinds.CONFIG_MAP)
            q = f"?watch=true&resourceVersion={rv0}&timeoutSeconds=60"
            nb_path = "/apis/kubeflow.org/{v}/namespaces/o/notebooks"
            cmw = await RawWatch(nat.port, CM.format(ns="o") + q).open()
            v1w = await RawWatch(nat.port, nb_path.format(v="v1") + q).open()
            betaw = await RawWatch(nat.port, nb_path.format(v="v1beta1") + q).open()
            watches = [cmw, v1w, betaw]
            for w in watches:
                await w.head()
            async with aiohttp.ClientSession() as s:
                async def call(method, path, body, ctype="application/json"):
                    async with s.request(method, nat.url + path, data=json.dumps(body), headers={"Content-Type": ctype}) as r:
                        assert r.status in (200, 201), await r.text()
                        return json.loads(await r.text())

                merge = "application/merge-patch+json"
                cm_out = [await call("POST", CM.format(ns="o"), configmap("c", "o", data={"a": "1"})),
                          await call("PATCH", CM.format(ns="o") + "/c", {"data": {"b": "é\n\"2\""}}, merge)]
                nb = notebook("nb", "o", image="img")
                nb["apiVersion"] = "kubeflow.org/v1"
                nb_out = [await call("POST", nb_path.format(v="v1"), nb),
                          await call("PATCH", nb_path.format(v="v1") + "/nb", {"metadata": {"labels": {"x": "y"}}}, merge),
                          await call("PATCH", nb_path.format(v="v1beta1") + "/nb/status", {"status": {"readyReplicas": 1, "conditions": [], "containerState": {}}}, merge)]
                assert [o["apiVersion"] for o in nb_out] == ["kubeflow.org/v1", "kubeflow.org/v1", "kubeflow.org/v1beta1"]

                # nothing committed: no event, the resourceVersion stays
                before = (await nat.stats())["resourceVersion"]
                dry = await call("POST", CM.format(ns="o") + "?dryRun=All", configmap("dry", "o"))
                assert dry["metadata"]["name"] == "dry"
                noop = await call("PATCH", CM.format(ns="o") + "/c", {"data": {"a": "1"}}, merge)
                assert noop == cm_out[1]
                assert (await nat.stats())["resourceVersion"] == before
                cm_out.append(await call("PATCH", CM.format(ns="o") + "/c", {"data": {"fence": "1"}}, merge))

            await asyncio.wait_for(cmw.read_until(lambda w: len(w.events) >= 3), 10)
            assert cmw.events == [("ADDED", cm_out[0]), ("MODIFIED", cm_out[1]), ("MODIFIED", cm_out[2])]
            for w, av in ((v1w, "kubeflow.org/v1"), (betaw, "kubeflow.org/v1beta1")):
                await asyncio.wait_for(w.read_until(lambda w: len(w.events) >= 3), 10)
                assert w.events == [(t, {**o, "apiVersion": av}) for t, o in zip(("ADDED", "MODIFIED", "MODIFIED"), nb_out)]
                # key order too: the line's object is the response's bytes
                assert [list(o) for _, o in w.events] == [list(o) for o in nb_out]
        finally:
            for w in watches:
                w.close()
            await c.close()
            await nat.stop()
    run(go(), timeout=60)


def test_webhook_cache_sees_configuration_changes(run):
    """The apiserver answers "which webhooks admit this write" from a cache: a change of the
    MutatingWebhookConfiguration between two creates is seen by the second, and deleting the
    configuration stops the admission calls."""
    from odh_kubeflow_amd.testing.cluster import ClusterConfig, LocalCluster

    async def go():
        cfg = ClusterConfig(odh=True, webhook=True, transport="native",
                            env={"SET_PIPELINE_RBAC": "false", "SET_PIPELINE_SECRET": "false"})
        async with LocalCluster(cfg) as cl:
            await cl.ensure_namespace("user")

            async def create_and_count(name):
                assert await cl.settle(10)
                before = cl.webhook.requests
                await cl.admin.create(notebook(name, "user"))
                assert await cl.settle(10)
                return cl.webhook.requests - before

            assert await create_and_count("nb0") >= 1  # cached from here on
            assert await create_and_count("nb1") >= 1
            mwc = (await cl.admin.list(kinds.MUTATING_WEBHOOK_CONFIGURATION))[0]
            shipped = mwc["webhooks"][0].get("matchConditions")
            mwc["webhooks"][0]["matchConditions"] = [{"name": "never", "expression": "false"}]
            mwc = await cl.admin.update(mwc)
            assert await create_and_count("nb2") == 0  # the very next create is no longer matched
            mwc["webhooks"][0]["matchConditions"] = shipped
            mwc["webhooks"][0]["rules"][0]["resources"] = ["configmaps"]
            mwc = await cl.admin.update(mwc)
            assert await create_and_count("nb3") == 0  # nor by rules that name another resource
            mwc["webhooks"][0]["rules"][0]["resources"] = ["notebooks"]
            mwc = await cl.admin.update(mwc)
            assert await create_and_count("nb4") >= 1  # and matched again
            await cl.admin.delete(kinds.MUTATING_WEBHOOK_CONFIGURATION, mwc["metadata"]["name"])
            assert await create_and_count("nb5") == 0
            assert await cl.admin.list(kinds.MUTATING_WEBHOOK_CONFIGURATION) == []
    run(go(), timeout=120)


def test_a_request_is_counted_before_it_is_answered(run):
    """5 creates and 5 patches, then /metrics on another connection, 20 times: the patch that was
    just answered is always counted."""
    async def go():
        nat, c = await start()
        try:
            await namespace(c, "m")
            for rnd in range(20):
                for i in range(5):
                    await c.create(configmap(f"c{rnd}-{i}", "m"))
                    await c.patch(kinds.CONFIG_MAP, {"data": {"k": str(i)}}, name=f"c{rnd}-{i}", namespace="m")
                prof = (await nat.stats())["prof"]
                assert prof["patch_calls"] % 5 == 0, prof["patch_calls"]
                assert prof["patch_calls"] == 5 * (rnd + 1) and prof["create_calls"] == 5 * (rnd + 1) + 1
            st = await nat.stats()
            assert set(st["phases"]) == {f"{p}_cpu_ns" for p in ("parse", "admit", "validate", "defaults", "patch",
                                                                 "prepare", "dump")}
            for k in ("watch_wakeups", "watch_scanned", "watch_gone", "watch_direct", "watch_fallback", "watch_slots"):
                assert k in st["prof"], k
        finally:
            await c.close()
            await nat.stop()
    run(go(), timeout=60)
