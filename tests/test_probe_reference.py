"""The host model of the probe kernels (``tests/probe_reference.py``) against itself, and the
shapes for which the probe's closed-form GEMM check says nothing.

The expected product of the probe operands depends only on ``K mod 35``: the full-period sum
is zero in every ``(i mod 5, j mod 7)`` class.  At ``K % 35 == 0`` the expectation is 0
everywhere, so a GPU whose matrix cores return zeros would pass; ``odh-gpu-probe`` and
``GpuProbe`` refuse such shapes.  No GPU is needed here.
"""

import os
import re

import numpy as np
import pytest

import probe_reference as ref
from odh_kubeflow_amd.ops import gpu

CSRC = os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "csrc")


def _cli_default_shape():
    with open(os.path.join(CSRC, "probe_cli.cpp"), encoding="utf-8") as f:
        m = re.search(r"struct Options \{\s*int M = (\d+), N = (\d+), K = (\d+);", f.read())
    return tuple(int(v) for v in m.groups())


@pytest.mark.parametrize("k", [32, 64, 96, 128, 192, 1024, 1120, 2240])
def test_closed_form_equals_integer_product(k):
    m, n = 75, 77  # more than two periods of both residues, neither a multiple of its period
    want = ref.probe_expected(m, n, k)
    assert np.array_equal(ref.probe_expected_closed_form(m, n, k), want)
    a, bt = ref.probe_operands(m, n, k)
    assert a.min() >= -2 and a.max() <= 2 and bt.min() >= -3 and bt.max() <= 3
    assert np.array_equal(a.astype(np.float64) @ bt.astype(np.float64).T, want.astype(np.float64))


def test_operands_follow_their_formulas():
    a, bt = ref.probe_operands(11, 13, 40)
    for i, k in ((0, 0), (1, 0), (0, 1), (10, 39), (7, 35)):
        assert a[i, k] == (3 * i + 7 * k) % 5 - 2
    for j, k in ((0, 0), (1, 0), (0, 1), (12, 39), (9, 35)):
        assert bt[j, k] == (11 * j + 5 * k) % 7 - 3


def test_shipped_probe_shapes_have_no_zero_class():
    assert ref.zero_classes(gpu.PROBE_SHAPE[2]) == 0
    cli = _cli_default_shape()
    assert cli == gpu.PROBE_SHAPE and ref.zero_classes(cli[2]) == 0
    assert ref.zero_classes(4096) == 11  # weaker, not vacuous


def test_class_table_is_all_zero_exactly_at_multiples_of_35():
    for k in range(32, 4481, 32):
        assert bool((ref.probe_class_table(k) == 0).all()) == (k % 35 == 0), k


def test_pattern_words_wrap_like_uint32():
    def scalar_mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16

    assert scalar_mix(0) == 0 and int(ref.mix32(np.uint32(0))) == 0
    for seed in (0, 0x9E3779B9, 0xFFFFFFFC, 0xFFFFFFFE):
        w = ref.pattern_words(5, seed)
        assert w.dtype == np.uint32 and w.shape == (20,)
        for i in range(5):
            b = (i * 4 & 0xFFFFFFFF) ^ seed
            assert [int(v) for v in w[4 * i:4 * i + 4]] == [scalar_mix(b + c & 0xFFFFFFFF) for c in range(4)]
    # 4 i keeps the low two bits of the seed, so b + c carries out of 32 bits only for a seed
    # whose low bits are not 00: 0xFFFFFFFE + 2 wraps to 0
    assert int(ref.pattern_words(1, 0xFFFFFFFE)[2]) == 0
    # element 2^30 has uint32(4 i) == 0 again
    assert ref.pattern_words(1, 7)[0] == ref.mix32(np.uint32(7))


def test_lcg_and_busy_model():
    assert ref.lcg(0) == 1013904223 and ref.lcg(0xFFFFFFFF) == (1013904223 - 1664525) & 0xFFFFFFFF
    out = ref.busy_expected()
    assert out.shape == (64,) and (out == 2304).all()


def test_fused_tile_id_is_a_bijection():
    for tiles_m, tiles_n, gm in ((2, 2, 1), (2, 2, 2), (2, 2, 4), (4, 1, 4), (8, 2, 8), (8, 2, 2), (6, 3, 4)):
        ids = sorted(ref.fused_tile_id(tm, tn, tiles_m, tiles_n, gm) for tm in range(tiles_m) for tn in range(tiles_n))
        assert ids == list(range(tiles_m * tiles_n))


def test_graph_and_eager_seeds_never_name_the_same_pattern():
    """The two start values differ in bit 31 alone and the LCG's multiplier is odd, so the orbits differ in
    bit 31 at every step; ``mix32`` is a bijection, so every word of the two patterns differs: a link checked
    against the wrong one of the two seeds counts every word."""
    assert ref.GRAPH_SEED0 ^ ref.EAGER_SEED0 == 1 << 31
    g, e = ref.lcg_sequence(ref.GRAPH_SEED0, 64), ref.lcg_sequence(ref.EAGER_SEED0, 64)
    assert g[0] == ref.lcg(ref.GRAPH_SEED0) and g[1] == ref.lcg(g[0]) and len(set(g)) == 64
    assert all(a ^ b == 1 << 31 for a, b in zip(g, e))
    assert (ref.pattern_words(4099, g[2]) != ref.pattern_words(4099, e[2])).all()


def test_harness_helpers():
    h = [0] * 32
    h[20], h[21] = -6, -1  # ~5 as two i32
    h[22], h[23] = 9, 1
    assert ref.graph_span(h, 20) == (5, (1 << 32) + 9) and ref.u64(h, 22) == (1 << 32) + 9
    assert ref.graph_span(h, 24) == (0xFFFFFFFFFFFFFFFF, 0)  # a span nothing stamped
    assert [ref.sweep_workgroups(n) for n in (1, 1024, 1025, 4096 * 1024, 1 << 30)] == [1, 1, 2, 4096, 4096]
    pos, xor = ref.link_flips(1000, 256, seed=3)
    assert len(set(pos.tolist())) == len(pos) and {0, 255, 256, 999} <= set(pos.tolist())
    assert pos.min() >= 0 and pos.max() < 1000 and (xor != 0).all() and xor.dtype == np.int32
    _, bt = ref.probe_operands(1, 512, 64)
    total, per_tile = ref.line_errors(bt, 37, 256)
    assert total == sum(per_tile) == int((bt[:, 37] != 0).sum()) and len(per_tile) == 2
    assert ref.errors_by_xcd([3, 4, 5], [7, 0, 7]) == [4, 0, 0, 0, 0, 0, 0, 8]
    assert ref.tile128_id(1, 2, 3) == 5


def test_gpu_probe_refuses_a_vacuous_shape():
    with pytest.raises(ValueError, match="35"):
        gpu.GpuProbe(0, 256, 256, 2240)
