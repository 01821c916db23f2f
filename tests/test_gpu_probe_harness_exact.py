"""The layer above the probe kernels on a real MI355X against the host model (``probe_reference.py``):
``GpuProbe.run()`` on every path it has, the captured graph behind it called through the ABI, the link
check of ``xgmi_ring_check`` between two probes on one GPU, and ``probe_devices``.

Every expectation is an exact integer.  The tests corrupt data only, inside buffers the kernels are
given in full, and put it back; every probe is closed, and at most two are alive at once.
"""

import ctypes

import numpy as np
import pytest

import probe_reference as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD_WORDS = 64  # int32 words on each side of a guarded buffer
GUARD = 0xA5A5A5A5 - (1 << 32)  # as int32
FILL = 0x5C5C5C5C
HIP_ERROR_INVALID_VALUE = 1
MIB = 1 << 20

ONE_TILE = (256, 256, 64)
FOUR_TILES = (512, 512, 64)  # per-XCD attribution needs more than one tile
NON_FUSED = (256, 384, 64)  # 2 × 3 tiles of 128²: the store kernel and the check kernel


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from odh_kubeflow_amd.ops import gpu

    gpu.load_library()  # loud failure if the in-tree .so is missing
    return torch.device("cuda", 0)


def _lib():
    from odh_kubeflow_amd.ops import gpu

    return gpu, gpu.load_library()


def _as_i32(words):
    return torch.from_numpy(words.view(np.int32))


# name -> (GpuProbe arguments, whether run() replays the graph, whether the shape is fused)
PATHS = {
    "graph": (dict(graph=True), True, True),
    "serial": (dict(graph="serial"), True, True),
    "eager-overlap": (dict(graph=False, overlap=True), False, True),
    "eager-sequential": (dict(graph=False, overlap=False), False, True),
    "eager-nontemporal": (dict(graph=False, hbm_nontemporal=True), False, True),
    "non-fused": (dict(), False, False),  # eager by construction
}
GRAPH_PATHS = [name for name, (_, graph, _) in PATHS.items() if graph]


def _probe(path, fused_shape, hbm_bytes=MIB):
    gpu, _ = _lib()
    kw, _, fused = PATHS[path]
    p = gpu.GpuProbe(0, *(fused_shape if fused else NON_FUSED), hbm_bytes=hbm_bytes, **kw)
    assert p.fused is fused
    return p


def _on_path(r, path):
    """The run took the path it was built for: a fall-back to the eager launches fails here."""
    _, graph, fused = PATHS[path]
    assert r["graph"] is graph, f"{path}: graph={r['graph']!r}, graph_error={r['graph_error']!r}"
    assert r["graph_error"] is None, r["graph_error"]
    assert r["fused_verify"] is fused


def _seed0(path):
    return ref.GRAPH_SEED0 if PATHS[path][1] else ref.EAGER_SEED0


# ------------------------------------------------------------------ a. the verdict, per path


def _run_fresh_map(p):
    p.tile_xcd.fill_(-1)  # so that the map read afterwards is this run's
    return p.run()


def _tile_map(p):
    gpu, _ = _lib()
    tx = p.tile_xcd.cpu().numpy()
    assert ((tx[:p.tiles] >= 0) & (tx[:p.tiles] < gpu.N_XCD)).all() and (tx[p.tiles:] == -1).all(), tx
    return tx


def _clean(p, r, path):
    gpu, _ = _lib()
    _on_path(r, path)
    assert r["ok"] is True, r
    assert r["gemm_errors"] == 0 and r["hbm_errors"] == 0, r
    tx = _tile_map(p)
    assert r["xcd_blocks"] == np.bincount(tx[:p.tiles], minlength=gpu.N_XCD).tolist()
    assert sum(r["xcd_blocks"]) == p.tiles
    assert r["err_xcd"] == [0] * gpu.N_XCD
    # the block as it came back: every error slot, the padding between them included
    assert p.host.tolist()[gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_HBM_ERR + 2] == [0] * 12


@pytest.mark.parametrize("path", list(PATHS))
def test_verdict_matches_host_model(dev, path):
    """Clean; one element of A off by one in the last tile-row; clean again with nothing carried over;
    the same with one element of Bt in the last tile-column.  The mismatches are the other operand's
    non-zeros at that k, and belong to the XCDs that ran the tiles of that row or column in that run."""
    gpu, _ = _lib()
    p = _probe(path, FOUR_TILES)
    try:
        m, n, k = p.m, p.n, p.k
        tile = 256 if p.fused else 128
        tiles_m, tiles_n = m // tile, n // tile
        assert p.tiles == tiles_m * tiles_n
        ha, hbt = ref.probe_operands(m, n, k)

        def tile_id(tm, tn):
            return ref.fused_tile_id(tm, tn, tiles_m, tiles_n) if p.fused else ref.tile128_id(tm, tn, tiles_n)

        _clean(p, _run_fresh_map(p), path)
        # (operand, its host copy, the other operand's host copy, line, k, tile ids along the line)
        cases = [(p.a, ha, hbt, m - 3, 37, [tile_id(tiles_m - 1, t) for t in range(tiles_n)]),
                 (p.bt, hbt, ha, n - 5, 22, [tile_id(t, tiles_n - 1) for t in range(tiles_m)])]
        for target, host, other, line, c, ids in cases:
            total, per_tile = ref.line_errors(other, c, tile)
            assert 0 < total < len(other)  # the case tells a check that counts from one that does not
            target[line, c] = float(host[line, c] + 1)  # exact in bf16: A -1..3, Bt -2..4
            try:
                r = _run_fresh_map(p)
            finally:
                target[line, c] = float(host[line, c])
            _on_path(r, path)
            tx = _tile_map(p)
            print(f"{path}: line {line}, k {c}: {r['gemm_errors']} counted, {total} expected; per XCD {r['err_xcd']}")
            assert r["gemm_errors"] == total
            assert r["err_xcd"] == ref.errors_by_xcd(per_tile, [tx[t] for t in ids])
            assert r["ok"] is False and r["hbm_errors"] == 0
            assert r["xcd_blocks"] == np.bincount(tx[:p.tiles], minlength=gpu.N_XCD).tolist()
            _clean(p, _run_fresh_map(p), path)
        for got, host in ((p.a, ha), (p.bt, hbt)):
            want = torch.from_numpy(host.astype(np.float32)).to(torch.bfloat16)
            assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    finally:
        p.close()


# ------------------------------------------------------------------ b. HBM contents and the pattern seed


def _holds_pattern(p, seed):
    got_seed = p.pattern_seed
    assert got_seed == seed, f"pattern_seed {got_seed if got_seed is None else hex(got_seed)}, expected {seed:#x}"
    got = p.hbm.cpu()
    want = _as_i32(ref.pattern_words(p.hbm_bytes // 16, seed))
    if not torch.equal(got, want):
        bad = (got != want).nonzero().flatten()
        pytest.fail(f"{bad.numel()} of {want.numel()} words are not the pattern of seed {seed:#x}, "
                    f"first at word {bad[0].item()}")


@pytest.mark.parametrize("path", list(PATHS))
def test_hbm_holds_the_pattern_of_pattern_seed(dev, path):
    p = _probe(path, ONE_TILE)
    try:
        assert p.pattern_seed is None  # nothing written yet
        for seed in ref.lcg_sequence(_seed0(path), 3):
            r = p.run()
            _on_path(r, path)
            assert r["ok"], r
            _holds_pattern(p, seed)
    finally:
        p.close()


def test_pattern_seed_follows_the_path_that_ran_last(dev):
    """Graph and eager runs keep seeds of their own; ``pattern_seed`` names the pattern in HBM after every
    run, across flips of ``graph``, and across ``close()`` and the re-capture after it."""
    p = _probe("graph", ONE_TILE)
    try:
        g = ref.lcg_sequence(ref.GRAPH_SEED0, 3)
        e = ref.lcg_sequence(ref.EAGER_SEED0, 2)
        for graph, seed in ((True, g[0]), (True, g[1]), (False, e[0]), (False, e[1]), (True, g[2])):
            p.graph = graph
            r = p.run()
            assert r["ok"] and r["graph"] is graph, r
            _holds_pattern(p, seed)
        p.close()
        _holds_pattern(p, g[2])  # the buffer is as the last replay left it
        r = p.run()  # captures again, with a fresh device-side seed
        assert r["ok"] and r["graph"] is True, r
        _holds_pattern(p, g[0])
    finally:
        p.close()


# ------------------------------------------------------------------ c. the graph through the ABI


def _guarded(dev, words, fill=FILL):
    """An int32 buffer of ``words`` payload words between two guards; returns (tensor, payload
    pointer = base + 256 bytes, 16-byte aligned)."""
    buf = torch.full((words + 2 * GUARD_WORDS,), fill, dtype=torch.int32, device=dev)
    buf[:GUARD_WORDS] = GUARD
    buf[GUARD_WORDS + words:] = GUARD
    ptr = buf.data_ptr() + 4 * GUARD_WORDS
    assert ptr % 16 == 0
    return buf, ptr


def _guards_intact(buf, words):
    return bool((buf[:GUARD_WORDS] == GUARD).all() and (buf[GUARD_WORDS + words:] == GUARD).all())


def _payload(buf, words):
    return buf[GUARD_WORDS:GUARD_WORDS + words]


class _GraphBuffers:
    """The test's own buffers for ``odh_probe_graph_create``: filled operands, and the HBM buffer, the
    counter block and the tile map between guards; a pinned host block with sentinels behind it."""

    SENTINEL = -7

    def __init__(self, dev, shape, hbm_bytes):
        gpu, lib = _lib()
        self.m, self.n, self.k = m, n, k = shape
        self.tiles = (m // 256) * (n // 256)
        self.hbm_bytes = hbm_bytes
        self.n16 = hbm_bytes // 16
        self.hbm_words = -(-hbm_bytes // 4)
        self.a = torch.empty((m, k), dtype=torch.bfloat16, device=dev)
        self.bt = torch.empty((n, k), dtype=torch.bfloat16, device=dev)
        gpu._check(lib.odh_probe_fill(self.a.data_ptr(), self.bt.data_ptr(), m, n, k,
                                      torch.cuda.current_stream().cuda_stream))
        self.hbm, self.hbm_ptr = _guarded(dev, self.hbm_words)
        self.counters, self.counters_ptr = _guarded(dev, gpu.ODH_NCOUNT)
        self.tile_xcd, self.tile_xcd_ptr = _guarded(dev, self.tiles, fill=-1)
        self.seed = torch.full((1,), ref.GRAPH_SEED0, dtype=torch.int32, device=dev)
        self.host = torch.full((2 * gpu.ODH_NCOUNT,), self.SENTINEL, dtype=torch.int32).pin_memory()
        torch.cuda.synchronize()

    def create(self, serial, out, **override):
        _, lib = _lib()
        a = dict(m=self.m, n=self.n, k=self.k, hbm_bytes=self.hbm_bytes)
        a.update(override)
        return lib.odh_probe_graph_create(self.a.data_ptr(), self.bt.data_ptr(), a["m"], a["n"], a["k"],
                                          self.tile_xcd_ptr, self.counters_ptr, self.hbm_ptr, a["hbm_bytes"],
                                          self.seed.data_ptr(), self.host.data_ptr(), serial, out)

    def untouched(self):
        gpu, _ = _lib()
        torch.cuda.synchronize()
        return bool((self.hbm[GUARD_WORDS:-GUARD_WORDS] == FILL).all() and (self.host == self.SENTINEL).all()
                    and (_payload(self.counters, gpu.ODH_NCOUNT) == FILL).all()
                    and (_payload(self.tile_xcd, self.tiles) == -1).all()
                    and int(self.seed.item()) == ref.GRAPH_SEED0)


# 16-byte elements 1, 1023, 1025 (and 8 bytes that belong to no element), 64·1024 + 1: 1, 1, 2 and 65
# workgroups, the last past the 64 that stamp the sweep's span from either end
GRAPH_HBM_BYTES = [16, 16 * 1023, 16 * 1025 + 8, 16 * (64 * 1024 + 1)]


def test_sweep_grid_of_the_graph_cases():
    assert [ref.sweep_workgroups(b // 16) for b in GRAPH_HBM_BYTES] == [1, 1, 2, 65]


@pytest.mark.parametrize("serial", [0, 1], ids=["parallel", "serial"])
@pytest.mark.parametrize("hbm_bytes", GRAPH_HBM_BYTES)
def test_graph_replay_at_the_edges_of_the_sweep_grid(dev, hbm_bytes, serial):
    gpu, lib = _lib()
    b = _GraphBuffers(dev, FOUR_TILES, hbm_bytes)
    h = ctypes.c_void_p()
    gpu._check(b.create(serial, ctypes.byref(h)))
    try:
        assert h.value
        stream = torch.cuda.Stream(dev)  # as GpuProbe replays it: on a stream of its own
        stream.wait_stream(torch.cuda.current_stream())
        for seed in ref.lcg_sequence(ref.GRAPH_SEED0, 2):
            gpu._check(lib.odh_probe_graph_launch(h, stream.cuda_stream))
            torch.cuda.synchronize()
            assert int(b.seed.item()) & 0xFFFFFFFF == seed
            want = torch.cat([_as_i32(ref.pattern_words(b.n16, seed)),
                              torch.full((b.hbm_words - 4 * b.n16,), FILL, dtype=torch.int32)])
            got = _payload(b.hbm, b.hbm_words).cpu()
            if not torch.equal(got, want):  # a tail that belongs to no element stays as it was
                bad = (got != want).nonzero().flatten()
                pytest.fail(f"{bad.numel()} wrong words, first at word {bad[0].item()} of {b.hbm_words}")
            assert _guards_intact(b.hbm, b.hbm_words)
            assert _guards_intact(b.counters, gpu.ODH_NCOUNT) and _guards_intact(b.tile_xcd, b.tiles)
            host = b.host.tolist()
            block = _payload(b.counters, gpu.ODH_NCOUNT).cpu().tolist()
            assert host[:gpu.ODH_NCOUNT] == block
            assert host[gpu.ODH_NCOUNT:] == [b.SENTINEL] * gpu.ODH_NCOUNT
            assert block[28:32] == [0] * 4
            # and the block says what a clean run says
            tx = _payload(b.tile_xcd, b.tiles).cpu().numpy()
            assert ((tx >= 0) & (tx < gpu.N_XCD)).all(), tx
            assert block[gpu.ODH_SLOT_XCD_BLOCKS:gpu.ODH_SLOT_XCD_BLOCKS + gpu.N_XCD] == np.bincount(
                tx, minlength=gpu.N_XCD).tolist()
            assert block[gpu.ODH_SLOT_ERR_XCD:gpu.ODH_SLOT_HBM_ERR + 2] == [0] * 12
            for slot in (gpu.ODH_SLOT_GRAPH_GEMM_SPAN, gpu.ODH_SLOT_GRAPH_SWEEP_SPAN):
                begin, end = ref.graph_span(block, slot)
                assert 0 < begin <= end, (slot, begin, end)
    finally:
        lib.odh_probe_graph_destroy(h)


def test_graph_create_refuses_and_clears_the_handle(dev):
    """No ``out``, a shape only the 128² tile divides, and less than one element of HBM: refused with
    ``hipErrorInvalidValue``, a handle variable that held something is NULL afterwards, nothing ran."""
    b = _GraphBuffers(dev, ONE_TILE, 16 * 1025)
    for serial in (0, 1):
        assert b.create(serial, None) == HIP_ERROR_INVALID_VALUE
        refused = [dict(m=NON_FUSED[0], n=128, k=NON_FUSED[2]), dict(k=32), dict(hbm_bytes=15), dict(hbm_bytes=0)]
        for override in refused:
            h = ctypes.c_void_p(0x5C5C5C50)  # never dereferenced: the call only overwrites it
            assert b.create(serial, ctypes.byref(h), **override) == HIP_ERROR_INVALID_VALUE, override
            assert h.value is None, (override, h.value)
    assert b.untouched()


# ------------------------------------------------------------------ d. spans are per replay


@pytest.mark.parametrize("path", GRAPH_PATHS)
def test_graph_spans_are_per_replay(dev, path):
    """Replays serialise on one stream and ``wall_clock64`` is monotonic, so a span begins no earlier than
    the one before it ended: no tolerance.  A block that is not reset keeps the first replay's start
    (``atomicMax`` on ``~begin``) and fails this."""
    gpu, lib = _lib()
    p = _probe(path, ONE_TILE)
    try:
        khz = lib.odh_wall_clock_khz(0) or 100000
        last = {}
        for replay in range(3):
            r = p.run()
            _on_path(r, path)
            h = p.host.tolist()
            for key, slot in (("gemm_ms", gpu.ODH_SLOT_GRAPH_GEMM_SPAN), ("hbm_ms", gpu.ODH_SLOT_GRAPH_SWEEP_SPAN)):
                begin, end = ref.graph_span(h, slot)
                print(f"{path} replay {replay} {key}: begin {begin} end {end} -> {r[key]} ms")
                assert 0 < begin <= end, (key, begin, end)
                assert last.get(key, 0) <= begin, f"{key}: replay {replay} begins at {begin}, before {last[key]}"
                last[key] = end
                assert r[key] == (end - begin) / khz
            assert r["ok"], r
    finally:
        p.close()


# ------------------------------------------------------------------ e. the link check on one GPU

LINK_SOURCE_BYTES = MIB + 16 * 1025  # no power of two, and no whole number of 1024-element slabs


def _link(pr, ps, nbytes):
    gpu, _ = _lib()
    lk = gpu.link_check(pr, ps, nbytes)
    assert lk["reader"] == 0 and lk["source"] == 0
    return lk


@pytest.mark.parametrize("path", list(PATHS))
def test_link_check_between_two_probes_on_one_gpu(dev, path):
    pr = _probe("graph", ONE_TILE)
    ps = None
    try:
        ps = _probe(path, ONE_TILE, hbm_bytes=LINK_SOURCE_BYTES)
        words = LINK_SOURCE_BYTES // 4
        lk = _link(pr, ps, 4 * MIB)  # a source that has never run: an error, not a verdict on its memory
        assert lk["ok"] is False and lk.get("error") and "errors" not in lk, lk
        seeds = ref.lcg_sequence(_seed0(path), 4)
        runs = 0

        def run_source():
            nonlocal runs
            r = ps.run()
            _on_path(r, path)
            assert r["ok"], r
            runs += 1
            assert ps.pattern_seed == seeds[runs - 1]

        run_source()
        for _ in range(2):  # after one run, and after three
            lk = _link(pr, ps, 4 * MIB)  # more than the buffer
            assert "error" not in lk, lk
            assert (lk["errors"], lk["bytes"], lk["ok"]) == (0, LINK_SOURCE_BYTES & ~15, True), lk
            part = 256 * 1024 + 8
            lk = _link(pr, ps, part)
            assert (lk["errors"], lk["bytes"], lk["ok"]) == (0, part & ~15, True), lk
            inside = (part & ~15) // 4
            pos, xor = ref.link_flips(words, inside, seed=1000 * runs + len(path))
            n_inside = int((pos < inside).sum())
            assert 0 < n_inside < len(pos)
            idx = torch.from_numpy(pos).to(dev)
            ps.hbm[idx] = ps.hbm[idx] ^ torch.from_numpy(xor).to(dev)
            lk = _link(pr, ps, part)
            assert (lk.get("errors"), lk["ok"]) == (n_inside, False), lk
            lk = _link(pr, ps, 4 * MIB)
            assert (lk.get("errors"), lk["ok"]) == (len(pos), False), lk
            run_source()  # a fresh pattern under a new seed, and the reader follows it
            lk = _link(pr, ps, 4 * MIB)
            assert (lk.get("errors"), lk["ok"]) == (0, True), lk
            if runs < 3:
                run_source()
        assert runs == 4
    finally:
        pr.close()
        if ps is not None:
            ps.close()


# ------------------------------------------------------------------ f. probe_devices on one GPU


def test_probe_devices_on_one_gpu(dev):
    """The process-wide probe of GPU 0 is left as found: its operands bit for bit."""
    gpu, _ = _lib()
    p = gpu.get_probe(0)
    before = (p.a.clone(), p.bt.clone())
    r = gpu.probe_devices([0])
    assert r["ok"] is True and r["error"] is None and "links" not in r, r
    i, c = p.m - 2, p.k - 1
    _, hbt = ref.probe_operands(1, p.n, p.k)
    total, _ = ref.line_errors(hbt, c, 256)
    clean = p.a[i, c].clone()
    p.a[i, c] = clean.float() + 1
    try:
        r = gpu.probe_devices([0])
    finally:
        p.a[i, c] = clean
    assert r["ok"] is False and r["error"] == "probe failed on GPU 0", r
    assert "links" not in r
    assert r["results"][0]["gemm_errors"] == total and r["results"][0]["ok"] is False
    r = gpu.probe_devices([0])
    assert r["ok"] is True and r["error"] is None and "links" not in r, r
    assert torch.equal(p.a.view(torch.int16), before[0].view(torch.int16))
    assert torch.equal(p.bt.view(torch.int16), before[1].view(torch.int16))
