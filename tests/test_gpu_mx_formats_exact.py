"""The BF8 / FP6 / BF6 block-scaled probe kernels on a real MI355X against the host model
(``mx_reference.py``): the BF8 instantiation and the 96-byte-row arms (FP6, BF6) of
``mx_gemm256_kernel`` (``gpu_probe_mx.h``) through ``odh_mx_gemm``, ``odh_mx_fill``,
``odh_mx_probe_gemm_verify`` and ``odh-gpu-probe --mx fp8,fp4,bf8,fp6,bf6``.

Nothing is written twice: each test calls the test of ``test_gpu_mx_exact.py`` of the same name, or
the sweep and store checks of ``probe_gpu.py`` that ``test_gpu_lowprec_sweeps.py`` runs, on these
three formats.  The file exists so that its cases keep the names they have always had.
"""

import pytest

import probe_gpu
import test_gpu_mx_exact as base
from probe_gpu import _gpu
from probe_gpu import _own_timeout, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FORMATS = ["bf8", "fp6", "bf6"]
ALL_FIVE = base.ALL_FIVE


@pytest.mark.parametrize("fmt,stages", [(f, s) for f in FORMATS for s in base.K_STAGES[f]])
def test_mx_gemm_exact_over_k(dev, fmt, stages):
    base._exact_store(dev, fmt, 256, 256, stages * base._stage(fmt))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", base.GRIDS)
def test_mx_gemm_exact_over_grids(dev, fmt, m, n):
    base._exact_store(dev, fmt, m, n, base._stage(fmt))


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_gemm_exact_over_tiles_and_stages(dev, fmt):
    """2 × 3 tiles at 3 stages: operand and scale addresses with a tile offset and ``kt > 0``."""
    base._exact_store(dev, fmt, 512, 768, 3 * base._stage(fmt))


def test_mx_entry_points_check_the_new_layouts(dev):
    gpu = _gpu()
    t = [base.torch.from_numpy(x).to(dev) for x in base._random_case("fp6", 256, 256, 128)[:4]]
    assert t[0].shape == (256, 96)
    assert tuple(gpu.mx_gemm("fp6", *t).shape) == (256, 256)  # the layout that is accepted
    with pytest.raises(ValueError):
        gpu.mx_gemm("bf8", *t)  # 96 bytes per row are no whole number of BF8 stages
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp6", t[0][:, :64].contiguous(), t[1][:, :64].contiguous(), *t[2:])  # rows of 64 bytes
    with pytest.raises(ValueError):
        gpu.mx_gemm("bf6", *t[:3], t[3][:, :2].contiguous())  # the scales are [256, 4]
    with pytest.raises(ValueError):
        gpu.mx_gemm("fp5", *t)


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_store_decodes_every_code_against_every_code(dev, fmt):
    probe_gpu.store_decodes_every_code(dev, fmt)


def test_fp6_store_applies_every_scale_byte(dev):
    probe_gpu.store_applies_every_scale_byte(dev, "fp6")


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_fill_matches_the_model(dev, fmt):
    base.test_mx_fill_matches_the_model(dev, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n,k", base.VERIFY_SHAPES)
def test_mx_verify_clean(dev, fmt, m, n, k):
    base.test_mx_verify_clean(dev, fmt, m, n, k)


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_verify_finds_a_corrupted_operand(dev, fmt):
    base.test_mx_verify_finds_a_corrupted_operand(dev, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_verify_reads_each_blocks_scale(dev, fmt):
    base.test_mx_verify_reads_each_blocks_scale(dev, fmt)


def test_mx_probe_reports_the_check(dev):
    base.test_mx_probe_reports_the_check(dev, FORMATS)


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_check_sees_every_row_and_column(dev, fmt, rows):
    probe_gpu.sweep_every_row_and_column(fmt, rows)


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_check_reads_every_scale_byte(dev, fmt, rows):
    probe_gpu.sweep_every_scale_byte(fmt, rows)


def test_program_checks_all_five_formats():
    """Everything on at once on one GPU: the verdict still fits the kubelet's 4096-byte termination
    message."""
    res, _ = base._program_passes(ALL_FIVE, "--dtypes", "f16,i8", "--rccl-mib", "16")
    assert set(res["dtypes"]) == {"f16", "i8"} and res["rccl"]["ok"] is True


def test_program_fails_every_format_on_injected_fault():
    base._program_fails_on_injected_fault(ALL_FIVE, 256, "--shape", "256,256,256")
