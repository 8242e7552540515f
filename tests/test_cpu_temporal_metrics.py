"""CPU side of test.py --metrics_temporal / ops.temporal_metrics: the float64 reference stated two ways agrees with itself and
with closed forms, its float32 evaluation is measured (the figures tests/test_gpu_temporal_metrics.py places its bound by),
the library exports and binds the entry points, and the host logic (options, summaries, pooling) does what the documents
say.  The kernels themselves: tests/test_gpu_temporal_metrics.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 8), (9, 37), (43, 70), (64, 64), (75, 133)]


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


@pytest.mark.parametrize("shape", SHAPES)
def test_vectorised_and_per_pixel_references_agree(shape):
    worst64, best32 = 0.0, float("inf")
    for seed in (1, 2, 3):
        for kind in ("noise", "smooth"):
            c = R.make_case(kind, *shape, seed=seed)          # (asserts min |margin| >= 1e-9)
            loop = R.reference_row_loop(*c["images"], c["f"], c["b"], c["fa"])
            for i in R.INTEGER_COLUMNS:
                assert loop[i] == c["row"][i], (kind, seed, R.COLUMNS[i])
            for i in R.FLOAT_COLUMNS:
                assert _rel(loop[i], c["row"][i]) <= 1e-13, (kind, seed, R.COLUMNS[i], loop[i], c["row"][i])
                worst64 = max(worst64, _rel(loop[i], c["row"][i]))
            r32 = R.reference_row(*c["images"], c["f"], c["b"], c["fa"], dtype=np.float32)
            best32 = min(best32, min(_rel(r32[i], c["row"][i]) for i in R.FLOAT_COLUMNS))
            inside, valid = R.fractions(c)
            # the fields exercise both outcomes of both tests: pixels leave the frame, and the mask rejects some that stay
            assert 0.7 <= inside <= 0.92 and 0.15 <= valid <= 0.85 and valid < inside, (kind, seed, inside, valid)
    # two float64 statements: <= 1.1e-14 on these cases; the float32 evaluation: never closer than 1.7e-9
    print("%dx%d: float64 loop vs vectorised <= %.1e; float32 vs float64 >= %.1e" % (shape + (worst64, best32)))
    assert best32 >= 1e-9


def test_box_rows_of_the_two_statements_agree():
    c = R.make_case("noise", 43, 70)
    for box in ((7, 40, 13, 60), (0, 31, 39, 70), (20, 21, 33, 34)):
        vec = R.reference_row(*c["images"], c["f"], c["b"], c["fa"], box)
        loop = R.reference_row_loop(*c["images"], c["f"], c["b"], c["fa"], box)
        assert [vec[i] for i in R.INTEGER_COLUMNS] == [loop[i] for i in R.INTEGER_COLUMNS]
        assert all(_rel(loop[i], vec[i]) <= 1e-13 for i in R.FLOAT_COLUMNS)
        assert vec[5] <= c["row"][5] and vec[0] <= c["row"][0]


def test_closed_forms():
    H, W = 20, 31
    rng = np.random.default_rng(5)
    img = rng.integers(0, 200, (H, W, 3), dtype=np.uint8)          # (<= 247: + 8 saturates nothing)
    other = rng.integers(0, 200, (H, W, 3), dtype=np.uint8)
    zero = np.zeros((H, W, 4), np.float32)
    for ref in (R.reference_row, R.reference_row_loop):
        # identical pairs, zero flows: every pixel valid, nothing differs
        assert ref(img, img, img, img, zero, zero, zero) == [H * W, 0.0, 0.0, H * W, 0.0, 0.0]
        # a == b: the generated pair IS the real pair
        c = R.make_case("smooth", 43, 70)
        _, _, b_cur, b_prev = c["images"]
        row = ref(b_cur, b_prev, b_cur, b_prev, c["f"], c["b"], c["f"])
        assert row[4] == 0.0 and row[1] == row[2] and row[5] == 0.0 and row[3] == 43 * 70 and 0 < row[0] < 43 * 70
        # + 8 on every byte of a_cur: the flicker term is 64 per value, exactly
        row = ref(img + 8, other, img, other, zero, zero, None)
        assert row[5] == 64 * 3 * H * W and row[3] == 0 and row[4] == 0.0 and row[0] == H * W
        assert row[1] == row[2] + 2 * 8 * float((img.astype(np.int64) - other).sum()) + 64 * 3 * H * W
    # a non-finite forward flow makes its pixel invalid and uncounted; a non-finite backward tap invalidates its readers
    f = zero.copy()
    f[3, 4, 0] = np.nan
    f[5, 6, 1] = np.inf
    f[7, 8, 0] = 1e30
    b = zero.copy()
    b[10, 10, 1] = -np.inf
    for ref in (R.reference_row, R.reference_row_loop):
        row = ref(img, img, img, img, f, b, zero)
        # 3 pixels by their own flow, 4 by the -Inf tap (weight 0 times Inf is NaN); 1e30 is finite: counted by n_flow
        assert row[0] == H * W - 7 and row[3] == H * W - 2
        assert row[4] == float(np.float32(1e30)) and row[1] == 0.0 and row[5] == 0.0


def test_library_exports_and_binding(lib_built):
    from text2video_amd import _lib
    assert lib_built.t2v_abi_version() == 22 == _lib.ABI_VERSION
    names = ("t2v_optical_flow_u8", "t2v_temporal_metrics_scratch_doubles", "t2v_temporal_metrics_u8")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "t2v.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and getattr(lib_built, name).argtypes == _lib.SIGNATURES[name][1]
        assert " T %s\n" % name in out
        # the header's declaration and the binding have the same number of parameters
        decl = re.findall(r"\b%s\(([^;]*)\);" % name, header)
        assert decl, name
        params = re.sub(r"/\*.*?\*/", "", decl[-1], flags=re.S)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "#define T2V_ABI_VERSION 22" in header and header.count("additive to ABI 22") >= 3
    assert "Sundaram" in header and "flow_a may be NULL" in header and "every flow this call returns is finite" in header
    # one partial per 32x16 tile, region and quantity; 0 for a shape the call refuses
    f = lib_built.t2v_temporal_metrics_scratch_doubles
    assert f(512, 512, 0) == 16 * 32 * 6 and f(75, 133, 3) == 5 * 5 * 4 * 6 and f(1, 1, 0) == 6
    assert f(0, 5, 0) == 0 and f(5, 0, 0) == 0 and f(8193, 5, 0) == 0 and f(5, 8193, 0) == 0 and f(5, 5, 4) == 0 and f(5, 5, -1) == 0


def test_metrics_temporal_option_implies_metrics_and_refuses_shard_chunks(capsys):
    from text2video_amd.options import TestOptions
    opt = TestOptions().parse([])
    assert opt.metrics is False and opt.metrics_temporal is False
    assert TestOptions().parse(["--metrics"]).metrics_temporal is False
    opt = TestOptions().parse(["--metrics_temporal"])
    assert opt.metrics is True and opt.metrics_temporal is True
    with pytest.raises(SystemExit):
        TestOptions().parse(["--metrics_temporal", "--shard_chunks"])
    assert "--metrics with --shard_chunks" in capsys.readouterr().err


def test_temporal_summary_and_pooling():
    from text2video_amd import metrics as M
    from text2video_amd import ops
    s = ops.temporal_summary([50.0, 300.0, 150.0, 80.0, 20.0, 1200.0], 100)
    assert s == {"warp_mse": 2.0, "warp_mse_real": 1.0, "valid": 0.5, "tof": 0.25, "tdiff_mse": 4.0}
    none = ops.temporal_summary([0.0, 0.0, 0.0, 0.0, 0.0, 30.0], 10)
    assert none["warp_mse"] is None and none["warp_mse_real"] is None and none["tof"] is None
    assert none["valid"] == 0.0 and none["tdiff_mse"] == 1.0
    assert isinstance(ops.TEMPORAL_DEFINITION, str) and "\n" not in ops.TEMPORAL_DEFINITION
    # pooled over sums, not a mean of ratios: (300 + 30) / (3 * (50 + 5)), not (2 + 2) / 2 ...
    rows = [np.array([50.0, 300.0, 150.0, 80.0, 20.0, 1200.0]), np.array([5.0, 30.0, 60.0, 20.0, 30.0, 0.0])]
    p = M.pool_temporal([(rows[0], 100), (rows[1], 100)])
    assert p == {"warp_mse": 2.0, "warp_mse_real": 210.0 / 165.0, "valid": 55.0 / 200.0, "tof": 0.5, "tdiff_mse": 2.0, "pairs": 2}
    assert M.pool_temporal([]) == {"warp_mse": None, "warp_mse_real": None, "valid": None, "tof": None, "tdiff_mse": None, "pairs": 0}
    # the document: frame 0 has no pair; a frame without a face has no face entry; without temporal rows no key exists
    frames = [("a.jpg", (10, 10), None), ("b.jpg", (10, 10), (0, 5, 0, 4)), ("c.jpg", (10, 10), None)]
    pic = np.tile(np.array([[300.0, 30.0, 45.0, 50.0]]), (6, 1))
    trows = np.full((6, 6), 9e99)                                   # (frame 0's rows and faceless face rows are never read)
    trows[2], trows[3], trows[4] = rows[0], [10.0, 60.0, 30.0, 20.0, 2.0, 120.0], rows[1]
    doc = M.summarise(frames, pic, trows)
    assert doc["frames"][0]["temporal"] is None
    assert doc["frames"][1]["temporal"] == dict(s, face={"warp_mse": 2.0, "warp_mse_real": 1.0, "valid": 0.5, "tof": 0.1, "tdiff_mse": 2.0})
    assert doc["frames"][2]["temporal"]["face"] is None and doc["frames"][2]["temporal"]["tof"] == 1.5
    assert doc["summary"]["temporal"] == dict(p, face=dict(doc["frames"][1]["temporal"]["face"], pairs=1))
    assert doc["temporal_definition"] == ops.TEMPORAL_DEFINITION
    plain = M.summarise(frames, pic)
    assert "temporal" not in plain["summary"] and all("temporal" not in f for f in plain["frames"]) and "temporal_definition" not in plain
    del doc["summary"]["temporal"], doc["temporal_definition"]
    for f in doc["frames"]:
        del f["temporal"]
    assert doc == plain


def test_metrics_and_evaluate_import_without_torch_on_the_lean_provider():
    """what a plain `test.py --metrics_temporal` run and `python -m text2video_amd.evaluate --temporal` import; and the views
    the one-buffer rows are made of exist on the lean provider's names"""
    code = ("import sys\nfrom text2video_amd import _xp\n_xp.use_lean()\nimport text2video_amd.metrics, text2video_amd.evaluate\n"
            "from text2video_amd import ops, leantorch\n"
            "assert callable(ops.temporal_metrics) and callable(ops.optical_flow_u8) and callable(ops.temporal_summary)\n"
            "assert hasattr(leantorch.Tensor, 'narrow') and hasattr(leantorch.Tensor, 'view')\n"
            "assert 'torch' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
