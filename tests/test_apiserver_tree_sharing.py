"""The native apiserver's object versions share what a write does not change (copy-on-write JSON
tree, ``testing/native/apiserver/json.hpp``), and validation skips what the stored version
already passed.  What must hold because of it:

* an old version never changes after a later write built on it — every kind of write, with more
  writes than the server keeps serialised lines for, so that old versions are serialised again
  from their trees;
* validation gives what walking the whole object gave: a wrongly typed status field is refused
  with the same message, an unknown status field is pruned, and the schema the server validates
  with is the one it started with, whatever is written to the CustomResourceDefinition object;
* concurrent patches of one object lose nothing, and every event is its write's response.
"""

import asyncio
import base64
import json

import pytest

from odh_kubeflow_amd.models import kinds
from odh_kubeflow_amd.models.errors import ApiError
from odh_kubeflow_amd.models.notebook import notebook
from odh_kubeflow_amd.runtime.rest import RestClient, RestConfig
from odh_kubeflow_amd.testing.apiserver import native

pytestmark = pytest.mark.skipif(not native.available(), reason="native apiserver not built")

NS = "tree"
LINE_KEEP = 64  # kLineKeep in apiserver.cpp: serialised lines kept per resource


def rv_of(obj) -> int:
    return int(obj["metadata"]["resourceVersion"])


async def start():
    nat = await native.NativeApiServer().start()
    c = RestClient(RestConfig(host=nat.url))
    await c.create({"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": NS}})
    return nat, c


def statefulset(name):
    return {"apiVersion": "apps/v1", "kind": "StatefulSet", "metadata": {"name": name, "namespace": NS, "labels": {"a": "1"}},
            "spec": {"serviceName": name, "selector": {"matchLabels": {"app": name}},
                     "template": {"metadata": {"labels": {"app": name}},
                                  "spec": {"containers": [{"name": "main", "image": "img:1",
                                                           "env": [{"name": "A", "value": "1"}, {"name": "B", "value": "2"}]},
                                                          {"name": "side", "image": "side:1"}]}}}}


class PatchingWebhook:
    """Answers every review of an object annotated ``mutate=yes`` with a JSON patch that adds,
    replaces and removes inside the first container's ``env`` array."""

    def __init__(self):
        self.requests = 0

    async def handle(self, review):
        self.requests += 1
        req = review["request"]
        resp = {"uid": req["uid"], "allowed": True}
        obj = req["object"]
        if (obj["metadata"].get("annotations") or {}).get("mutate") == "yes":
            patch = [{"op": "add", "path": "/spec/template/spec/containers/0/env/-", "value": {"name": "HOOKED", "value": "1"}},
                     {"op": "replace", "path": "/spec/template/spec/containers/0/env/0/value", "value": "by-webhook"},
                     {"op": "remove", "path": "/metadata/annotations/mutate"}]
            resp["patchType"] = "JSONPatch"
            resp["patch"] = base64.b64encode(json.dumps(patch).encode()).decode()
        return {"apiVersion": "admission.k8s.io/v1", "kind": "AdmissionReview", "response": resp}


async def replay(c, kind, since: int, until: int):
    """The events of ``kind`` in NS after resourceVersion ``since`` up to ``until``."""
    out = []
    async for etype, obj in c.watch(kind, NS, resource_version=str(since), timeout_s=5, bookmarks=False):
        out.append((etype, obj))
        if rv_of(obj) >= until:
            break
    return out


def test_old_versions_do_not_change(run):
    """One write of every kind on a Notebook and a StatefulSet, then more status patches than the
    server keeps serialised lines; a watch from the creation replays every version, and each
    must be the response recorded when it was written."""
    from odh_kubeflow_amd.webhook.certs import generate
    from odh_kubeflow_amd.webhook.server import WebhookServer, mutating_webhook_configuration

    async def go():
        nat, c = await start()
        hook = PatchingWebhook()
        certs = generate(("127.0.0.1", "localhost"))
        wh = await WebhookServer(hook, certs.cert_dir, "127.0.0.1", 0).start()
        try:
            await c.create(mutating_webhook_configuration(certs.ca_bundle_b64, url=f"https://127.0.0.1:{wh.port}/mutate-notebook-v1"))
            nb_out, sts_out = [], []  # every response, in order
            nb0 = notebook("nb", NS, annotations={"keep": "1"})
            nb0["spec"]["template"]["spec"]["containers"][0]["env"] = [{"name": "A", "value": "1"}, {"name": "B", "value": "2"}]
            nb_out.append(await c.create(nb0))
            sts_out.append(await c.create(statefulset("sts")))

            async def both(patch_nb, patch_sts, ptype="merge", sub=None):
                nb_out.append(await c.patch(kinds.NOTEBOOK, patch_nb, ptype, name="nb", namespace=NS, subresource=sub))
                sts_out.append(await c.patch(kinds.STATEFUL_SET, patch_sts, ptype, name="sts", namespace=NS, subresource=sub))

            # a merge patch on spec
            await both({"spec": {"template": {"spec": {"serviceAccountName": "sa"}}}}, {"spec": {"replicas": 2}})
            # a status merge patch
            cond = {"type": "Ready", "status": "True", "lastProbeTime": "2026-01-01T00:00:00Z"}
            await both({"status": {"readyReplicas": 1, "conditions": [cond], "containerState": {"running": {"startedAt": "t0"}}}},
                       {"status": {"replicas": 2, "readyReplicas": 1}}, sub="status")
            # a JSON patch that adds, removes and replaces inside an array
            ops = [{"op": "add", "path": "/spec/template/spec/containers/0/env/-", "value": {"name": "C", "value": "3"}},
                   {"op": "replace", "path": "/spec/template/spec/containers/0/env/0/value", "value": "one"},
                   {"op": "remove", "path": "/spec/template/spec/containers/0/env/1"}]
            await both(ops, ops, "json")
            # a strategic patch on a keyed list (containers by name)
            await both({"spec": {"template": {"spec": {"containers": [{"name": "nb", "image": "img:2"}]}}}},
                       {"spec": {"template": {"spec": {"containers": [{"name": "side", "image": "side:2"},
                                                                      {"name": "third", "image": "third:1"}]}}}}, "strategic")
            assert [x["name"] for x in sts_out[-1]["spec"]["template"]["spec"]["containers"]] == ["main", "side", "third"]
            # a PUT
            for kind, outs in ((kinds.NOTEBOOK, nb_out), (kinds.STATEFUL_SET, sts_out)):
                cur = await c.get(kind, outs[-1]["metadata"]["name"], NS)
                assert cur == outs[-1]
                cur["metadata"]["labels"] = {**(cur["metadata"].get("labels") or {}), "put": "yes"}
                outs.append(await c.update(cur))
            # an update mutated by the registered webhook's JSON patch
            before = hook.requests
            cur = json.loads(json.dumps(nb_out[-1]))
            cur["metadata"]["annotations"]["mutate"] = "yes"
            nb_out.append(await c.update(cur))
            assert hook.requests == before + 1
            env = nb_out[-1]["spec"]["template"]["spec"]["containers"][0]["env"]
            assert env[0] == {"name": "A", "value": "by-webhook"} and env[-1] == {"name": "HOOKED", "value": "1"}
            assert "mutate" not in nb_out[-1]["metadata"]["annotations"] and nb_out[-1]["metadata"]["annotations"]["keep"] == "1"
            # more writes than serialised lines are kept for: old versions are serialised again
            for i in range(LINE_KEEP + 6):
                await both({"status": {"readyReplicas": i % 3, "conditions": [{**cond, "message": f"m{i}"}]}},
                           {"status": {"readyReplicas": i % 3, "observedGeneration": i}}, sub="status")
            assert await c.get(kinds.NOTEBOOK, "nb", NS) == nb_out[-1]
            # a finalizer removal on a deleting object
            for kind, name, outs in ((kinds.NOTEBOOK, "nb", nb_out), (kinds.STATEFUL_SET, "sts", sts_out)):
                outs.append(await c.patch(kind, {"metadata": {"finalizers": ["tests/hold"]}}, name=name, namespace=NS))
            nb_out.append(await c.delete(kinds.NOTEBOOK, "nb", NS))
            assert nb_out[-1]["metadata"].get("deletionTimestamp")
            nb_out.append(await c.patch(kinds.NOTEBOOK, {"metadata": {"finalizers": None}}, name="nb", namespace=NS))

            for kind, outs in ((kinds.NOTEBOOK, nb_out), (kinds.STATEFUL_SET, sts_out)):
                rvs = [rv_of(o) for o in outs]
                assert all(a < b for a, b in zip(rvs, rvs[1:])), "every write made a new version"
                events = await asyncio.wait_for(replay(c, kind, rvs[0], rvs[-1]), 30)
                assert [rv_of(o) for _t, o in events] == rvs[1:]
                for (etype, obj), want in zip(events, outs[1:]):
                    assert obj == want, f"version {rv_of(want)} changed after it was written"
                    assert list(obj) == list(want) and list(obj["metadata"]) == list(want["metadata"])  # member order
                types = [t for t, _o in events]
                assert set(types[:-1]) == {"MODIFIED"}
                assert types[-1] == ("DELETED" if kind == kinds.NOTEBOOK else "MODIFIED")
            assert await c.get(kinds.STATEFUL_SET, "sts", NS) == sts_out[-1]
            with pytest.raises(ApiError):
                await c.get(kinds.NOTEBOOK, "nb", NS)
        finally:
            await wh.stop()
            await c.close()
            await nat.stop()
    run(go(), timeout=120)


# What the parent commit's server answers to the write below (recorded from its binary); the
# single-walk validation must word it the same.
WRONG_TYPE_MESSAGE = ('Notebook.kubeflow.org "nb" is invalid: status.readyReplicas: Invalid value: "three": '
                      'status.readyReplicas in body must be of type integer: "string"')


MISSING_IN_ITEM_MESSAGE = 'Notebook.kubeflow.org "nb" is invalid: status.conditions[1].status: Required value'


def test_validation_is_unchanged(run):
    """Status writes are validated, pruned and defaulted as a walk of the whole object did."""
    async def go():
        nat, c = await start()
        try:
            created = await c.create(notebook("nb", NS))
            good = {"type": "Ready", "status": "True"}
            full = {"conditions": [good], "containerState": {}, "readyReplicas": 0}  # the schema requires all three
            await c.patch(kinds.NOTEBOOK, {"status": full}, name="nb", namespace=NS, subresource="status")
            # a wrongly typed field: refused, with the message the parent gives
            for write in (lambda: c.patch(kinds.NOTEBOOK, {"status": {"readyReplicas": "three"}}, name="nb", namespace=NS,
                                          subresource="status"),
                          lambda: c.update_status({**created, "status": {**full, "readyReplicas": "three"}})):
                with pytest.raises(ApiError) as e:
                    await write()
                assert e.value.code == 422 and e.value.message == WRONG_TYPE_MESSAGE, e.value.message
            # deeper, inside an array item that sits beside an unchanged one
            with pytest.raises(ApiError) as e:
                await c.patch(kinds.NOTEBOOK, [{"op": "add", "path": "/status/conditions/-", "value": {"type": "X"}}], "json",
                              name="nb", namespace=NS, subresource="status")
            assert e.value.message == MISSING_IN_ITEM_MESSAGE, e.value.message
            # an unknown field in a patched status is pruned, beside what stays
            out = await c.patch(kinds.NOTEBOOK, {"status": {"bogus": 1, "readyReplicas": 2,
                                                            "containerState": {"running": {"startedAt": "t", "nope": 1}}}},
                                name="nb", namespace=NS, subresource="status")
            assert out["status"] == {"conditions": [good], "readyReplicas": 2, "containerState": {"running": {"startedAt": "t"}}}
            assert out["spec"] == created["spec"]
            # The schema is read when the server starts; writing a stricter one into the
            # CustomResourceDefinition object replaces nothing (the parent commit answers the
            # write below with 200 as well: established against its binary).  So an object
            # stored under the start-up schema takes a status-only write afterwards exactly as
            # before, and a spec the stricter schema would refuse is still accepted.
            from odh_kubeflow_amd.models.crd import notebook_crd

            crd = notebook_crd()
            await c.create(crd)
            for v in crd["spec"]["versions"]:
                st = v["schema"]["openAPIV3Schema"]["properties"]["status"]
                st["properties"]["readyReplicas"] = {"type": "integer", "maximum": 0}
                st["required"] = ["neverThere"]
            await c.update({**crd, "metadata": (await c.get(kinds.CRD, crd["metadata"]["name"]))["metadata"]})
            out2 = await c.patch(kinds.NOTEBOOK, {"status": {"readyReplicas": 5}}, name="nb", namespace=NS, subresource="status")
            assert out2["status"]["readyReplicas"] == 5 and rv_of(out2) > rv_of(out)
            with pytest.raises(ApiError) as e:
                await c.patch(kinds.NOTEBOOK, {"status": {"readyReplicas": "three"}}, name="nb", namespace=NS, subresource="status")
            assert e.value.message == WRONG_TYPE_MESSAGE
        finally:
            await c.close()
            await nat.stop()
    run(go(), timeout=60)


def test_concurrent_patches_of_one_object(run):
    """Eight clients patch disjoint labels and status fields of one Notebook, 50 times each, with
    no precondition, two watchers open: nothing is lost, each stream's resourceVersions rise
    strictly, and each event is the response of its write."""
    async def go():
        nat, c = await start()
        clients = [RestClient(RestConfig(host=nat.url)) for _ in range(8)]
        try:
            await c.create(notebook("nb", NS))
            # the Notebook status schema has exactly eight scalar leaves besides the conditions: one per writer
            leaves = [("containerState", "waiting", "message"), ("containerState", "waiting", "reason"),
                      ("containerState", "running", "startedAt"), ("containerState", "terminated", "containerID"),
                      ("containerState", "terminated", "message"), ("containerState", "terminated", "reason"),
                      ("containerState", "terminated", "finishedAt"), ("readyReplicas",)]

            def status_field(w, i):
                out = i + 1 if leaves[w] == ("readyReplicas",) else str(i + 1)  # never the value it has: no no-op writes
                for k in reversed(leaves[w]):
                    out = {k: out}
                return out

            def merge(into, patch):
                for k, v in patch.items():
                    if isinstance(v, dict):
                        into[k] = merge(dict(into.get(k) or {}), v)
                    else:
                        into[k] = v
                return into

            first = await c.patch(kinds.NOTEBOOK, {"status": {"conditions": [], "readyReplicas": 0,
                                                              "containerState": {"terminated": {"exitCode": 0}}}},
                                  name="nb", namespace=NS, subresource="status")
            created = first
            responses = {}

            async def watcher():
                seen = []
                async for etype, obj in c.watch(kinds.NOTEBOOK, NS, resource_version=str(rv_of(created)), timeout_s=30,
                                                bookmarks=False):
                    seen.append((etype, obj))
                    if len(seen) >= 8 * 50:
                        break
                return seen

            watchers = [asyncio.ensure_future(watcher()) for _ in range(2)]

            async def writer(w, cl):
                for i in range(50):
                    while True:
                        try:
                            if i % 2:
                                out = await cl.patch(kinds.NOTEBOOK, {"metadata": {"labels": {f"w{w}": str(i)}}}, name="nb",
                                                     namespace=NS)
                            else:
                                out = await cl.patch(kinds.NOTEBOOK, {"status": status_field(w, i)}, name="nb", namespace=NS,
                                                     subresource="status")
                            break
                        except ApiError as e:
                            # the server re-applies an unconditional patch to the live version a bounded
                            # number of times; eight writers on a slow build can use them up, and a client
                            # then does what the message says
                            if e.reason != "Conflict":
                                raise
                    responses[rv_of(out)] = out

            await asyncio.gather(*(writer(w, cl) for w, cl in enumerate(clients)))
            final = await c.get(kinds.NOTEBOOK, "nb", NS)
            want_status = dict(first["status"])
            for w in range(8):
                assert final["metadata"]["labels"][f"w{w}"] == "49"
                merge(want_status, status_field(w, 48))
            assert final["status"] == want_status
            assert len(responses) == 8 * 50
            for fut in watchers:
                seen = await asyncio.wait_for(fut, 60)
                rvs = [rv_of(o) for _t, o in seen]
                assert all(a < b for a, b in zip(rvs, rvs[1:]))
                mine = [(t, o) for t, o in seen if rv_of(o) in responses]
                assert len(mine) == 8 * 50
                for _t, o in mine:
                    assert o == responses[rv_of(o)]
            assert final == responses[max(responses)]
        finally:
            for cl in clients:
                await cl.close()
            await c.close()
            await nat.stop()
    run(go(), timeout=120)
