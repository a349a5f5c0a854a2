"""Scale-invariant boundary metric (csrc/dp_boundary.hip, depth_pro/eval/boundary_metrics.py).

The expected values are the reference's own: tests/golden/golden_boundary.npz holds, per case, what the reference's
fgbg_depth, fgbg_depth_thinned, fgbg_binary_mask, SI_boundary_F1 and SI_boundary_Recall return (made by
tests/golden/make_golden_boundary.py, which lists the cases and asserts their properties).  tests/boundary_numpy.py
restates the header's rules in vectorised numpy; the non-GPU tests pin it to the golden file, the GPU tests compare the
device with the golden file.  Counts and maps are integers and are compared exactly.  Scores are compared exactly when
numpy is the version that made the golden file; otherwise within 18 * 2^-53: the per-threshold scores come from the
same integer counts through the same float64 expressions, so only numpy's order of summing the 10 products
score_k * weight_k can differ, and two orderings of a 10-term sum of terms bounded by the weights (which sum to 1)
differ by at most 2 * 9 * 2^-53.
"""

import ctypes
import json
import os
import sys

import numpy as np
import pytest

import boundary_numpy as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORE_TOL = 18 * 2.0 ** -53
ARG, SHAPE = 1000, 1001


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_boundary.npz"))


@pytest.fixture(scope="module")
def names(gold):
    return [str(n) for n in gold["names"]]


def _case(gold, name):
    return gold[f"{name}_pred"], gold[f"{name}_target"], gold[f"{name}_alpha"]


def _maps(gold, name, which, k):
    shape = gold[f"{name}_pred"].shape
    return np.unpackbits(gold[f"{name}_{which}_{k}"])[:4 * shape[0] * shape[1]].reshape((4,) + shape)


def _same_score(got, want, gold):
    if np.__version__ == str(gold["numpy_version"]):
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= SCORE_TOL, (got, want)


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_golden_file_holds_the_cases(gold, names):
    shapes = {tuple(gold[f"{n}_pred"].shape) for n in names}
    L = 64
    assert shapes >= {(1, 1), (1, 2), (2, 1), (1, 70), (70, 1), (37, 64), (37, 65), (37, 66), (65, 37), (66, 37), (3, 257), (257, 3),
                      (4, 2 * L + 1), (4, 2 * L + 2), (2 * L + 1, 4), (2 * L + 2, 4), (97, 131)}      # lines of L, L + 1, 2 L + 1 cells and places
    assert list(gold["thresholds"]) == list(np.linspace(1.05, 1.25, 10)) and list(gold["map_k"]) == [1, 7]
    assert (gold["scene_plain"] > 0).all() and (gold["scene_thin"] > 0).all()
    assert (gold["whole_5x66_thin"][:, 2, 2] == 5).all() and (gold["whole_66x5_thin"][:, 3, 2] == 5).all()
    assert gold["width_plain"][1, 0, 2] == 1 and gold["width_thin"][1, 0, 2] == 0       # the two compare widths


def test_restatement_equals_the_reference(gold, names):
    th = gold["thresholds"]
    for name in names:
        pred, tgt, alpha = _case(gold, name)
        pi = B.invert_depth(pred)
        assert np.array_equal(B.counts(pi, B.invert_depth(tgt), th, "depth", "f64"), gold[f"{name}_plain"]), name
        assert np.array_equal(B.counts(pi, alpha > 0.1, th, "mask", "f32"), gold[f"{name}_thin"]), name
        for k in gold["map_k"]:
            assert np.array_equal(B.padded(B.plain_edges(pi, th[k], "f64"), pred.shape), _maps(gold, name, "pmap", k)), (name, k)
            assert np.array_equal(B.padded(B.thinned_edges(pi, th[k], "f32"), pred.shape), _maps(gold, name, "tmap", k)), (name, k)
        _same_score(B.si_boundary_f1(pred, tgt), float(gold[f"{name}_f1"]), gold)
        _same_score(B.si_boundary_recall(pred, alpha), float(gold[f"{name}_recall"]), gold)


def test_rounded_threshold_in_double_is_the_float32_comparison(gold):
    """What the recall wrapper relies on: (double)ratio > (double)(float)t is ratio > float32(t)."""
    th = gold["thresholds"]
    for name in ("width", "scene", "special"):
        pi = B.invert_depth(gold[f"{name}_pred"])
        m = gold[f"{name}_alpha"] > 0.1
        assert np.array_equal(B.counts(pi, m, th.astype(np.float32).astype(np.float64), "mask", "f64"), gold[f"{name}_thin"]), name
    assert np.float32(th[1]) > th[1] and sum(float(np.float32(t)) > t for t in th) >= 4


def test_score_expressions_of_the_package(gold, names):
    from depth_pro.eval import boundary_metrics as M

    th, w = M.get_thresholds_and_weights(1.05, 1.25, 10)
    assert np.array_equal(th, gold["thresholds"]) and np.array_equal(w, th / th.sum())
    for name in names:
        _same_score(M.weighted_score(gold[f"{name}_plain"].astype(np.int64).tolist(), th, M.DP_BOUNDARY_DEPTH), float(gold[f"{name}_f1"]), gold)
        _same_score(M.weighted_score(gold[f"{name}_thin"].astype(np.int64).tolist(), th, M.DP_BOUNDARY_MASK), float(gold[f"{name}_recall"]), gold)
    zero = [[0, 0, 0]] * 4
    assert M.f1_from_counts(zero) == 0.0 and M.f1_from_counts(zero, return_p=True) == 0.0 and M.recall_from_counts(zero) == 0.0
    c = [[1, 2, 4], [0, 0, 0], [3, 3, 3], [0, 5, 0]]
    r, p = 0.25 * (1 / 2 + 0 / 1 + 3 / 3 + 0 / 5), 0.25 * (1 / 4 + 0 / 1 + 3 / 3 + 0 / 1)
    assert (M.f1_from_counts(c, return_r=True), M.f1_from_counts(c, return_p=True), M.f1_from_counts(c)) == (r, p, 2 * (r * p) / (r + p))
    d = np.array([[np.nan, 0.0, -1.0, 1e-7, 2.0, np.inf]], np.float32)
    assert np.array_equal(M.invert_depth(d), B.invert_depth(d), equal_nan=True) and M.invert_depth(d).dtype == np.float32


def test_abi_is_additive():
    import re

    from depth_pro import _lib

    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dp_mi355x.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t) (dp_boundary_\w+)\(", src, flags=re.M))
    assert declared == {"dp_boundary_workspace_size", "dp_boundary_counts", "dp_boundary_edges"} and declared <= set(_lib.EXPORTS)
    assert _lib.DP_ABI_VERSION == 20 and "#define DP_ABI_VERSION 20" in src
    for name in ("MAX_DIM", "MAX_T", "DIRS", "COUNTS", "DEPTH", "MASK", "INVERSE", "SEGMENT"):
        assert int(re.search(rf"^#define DP_BOUNDARY_{name}\s+(\d+)", src, flags=re.M).group(1)) == getattr(_lib, f"DP_BOUNDARY_{name}")
    lib = _lib.load()
    assert lib.dp_abi_version() == 20


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    size = lib.dp_boundary_workspace_size
    sizes = [size(64, 64, 1), size(64, 65, 1), size(64, 66, 1), size(64, 66, 10), size(64, 66, 17), size(1536, 1536, 10)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and size(1, 1, 1) > 0 and size(0, 5, 1) == size(1, 1, 1)
    assert size(16384, 16384, 32) > 2 ** 32
    P, big = 4096, 1 << 44
    th = (ctypes.c_double * 32)(*np.linspace(1.05, 1.25, 32))

    def counts(pred=P, ldp=40, tgt=P, ldt=40, kind=0, H=30, W=40, t=th, n=10, out=P, ws=P, wsb=big):
        return lib.dp_boundary_counts(pred, ldp, tgt, ldt, kind, H, W, t, n, out, ws, wsb, None)

    def edges(depth=P, ld=40, H=30, W=40, t=1.1, thinned=1, maps=P, ws=P, wsb=big):
        return lib.dp_boundary_edges(depth, ld, H, W, t, thinned, maps, ws, wsb, None)

    for kw in ({"pred": None}, {"tgt": None}, {"t": None}, {"out": None}, {"ws": None}, {"out": P + 4}, {"ws": P + 2},
               {"wsb": size(30, 40, 10) - 1}, {"wsb": 0}, {"kind": 4}, {"kind": 8}, {"kind": -1}):
        assert counts(**kw) == ARG, kw
    for kw in ({"H": 0}, {"W": 0}, {"H": 16385}, {"W": 16385}, {"H": -3}, {"n": 0}, {"n": 33}, {"ldp": 39}, {"ldt": 39}):
        assert counts(**kw) == SHAPE, kw
    for bad in (float("nan"), float("inf"), float("-inf")):
        t = (ctypes.c_double * 3)(1.05, bad, 1.2)
        assert counts(t=t, n=3) == ARG and counts(t=t, n=1) != ARG and edges(t=bad) == ARG, bad
    for kw in ({"depth": None}, {"maps": None}, {"ws": None}, {"ws": P + 1}, {"wsb": size(30, 40, 1) - 1}):
        assert edges(**kw) == ARG, kw
    for kw in ({"H": 0}, {"W": 16385}, {"ld": 39}):
        assert edges(**kw) == SHAPE, kw
    with pytest.raises(_lib.DPError, match="DP_ERR_ARG"):
        _lib.check(counts(kind=4), "dp_boundary_counts")


def test_wrappers_refuse_bad_arguments_and_host_tensors():
    import torch

    from depth_pro import _lib
    from depth_pro.eval import boundary_metrics as M

    d = torch.ones(5, 7)
    for call in (lambda: M.boundary_counts(d, d, [1.1]), lambda: M.boundary_edges(d, 1.1), lambda: M.boundary_edges(d, 1.1, True),
                 lambda: M.boundary_counts(d, d > 0, [1.1], M.DP_BOUNDARY_MASK), lambda: M.SI_boundary_F1(d, d),
                 lambda: M.SI_boundary_Recall(d, d > 0), lambda: M.boundary_f1(d, d, 1.1), lambda: M.edge_recall_matting(d, d > 0, 1.1)):
        with pytest.raises(_lib.DPError):
            call()
    f64 = np.ones((5, 7))
    f32 = np.ones((5, 7), np.float32)
    for call in (lambda: M.SI_boundary_F1(f64, f64), lambda: M.SI_boundary_F1(d.double(), d.double()), lambda: M.SI_boundary_F1(d[0], d[0]),
                 lambda: M.SI_boundary_F1(d[None], d[None]), lambda: M.SI_boundary_F1(d, torch.ones(5, 8)), lambda: M.SI_boundary_F1(d, d, N=0),
                 lambda: M.SI_boundary_Recall(d, d, N=0), lambda: M.SI_boundary_Recall(d, d.to(torch.int32)), lambda: M.SI_boundary_Recall(d.half(), d),
                 lambda: M.SI_boundary_Recall(f32, np.ones((5, 7), np.int64)), lambda: M.SI_boundary_F1(f32, f64), lambda: M.boundary_edges(f64, 1.1),
                 lambda: M.boundary_edges(d, float("nan")), lambda: M.boundary_counts(d, d, []), lambda: M.boundary_counts(d, d, [1.0] * 33),
                 lambda: M.boundary_counts(d, d, [float("inf")]), lambda: M.boundary_counts(d, d, [1.1], 7), lambda: M.SI_boundary_F1(d, d, N=33),
                 lambda: M.SI_boundary_F1([[1.0]], [[1.0]]), lambda: M.edge_recall_matting(d, d, 1.1), lambda: M.get_thresholds_and_weights(1, 2, 0)):
        with pytest.raises(ValueError):
            call()


def test_cli_flag_and_resume_planning(tmp_path, monkeypatch):
    import generate_depth_maps as G

    monkeypatch.setattr(G, "_model", lambda *a, **k: pytest.fail("the model was loaded"))
    notdir = tmp_path / "file.npy"
    notdir.write_bytes(b"")
    for bad in (str(tmp_path / "missing"), str(notdir)):
        monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--boundary_dir", bad])
        with pytest.raises(SystemExit) as e:
            G.main()
        assert e.value.code == 2, bad
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), boundary_dir=str(tmp_path / "missing"))
    frames = [str(tmp_path / f"f{k}.png") for k in range(3)]
    assert G.boundary_name(frames[0]) == "f0_boundary.json"
    tdir = tmp_path / "targets"
    tdir.mkdir()
    np.save(tdir / "f0.npy", np.ones((2, 2), np.float32))
    np.save(tdir / "f1.npy", np.ones((2, 2), np.float32))
    for k in range(3):
        (tmp_path / f"f{k}_depth.png").write_bytes(b"")
    (tmp_path / "f0_boundary.json").write_bytes(b"{}")
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True) == []
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, boundary=str(tdir)) == [1]      # f1 has a target and no JSON; f2 has no target
    assert G.plan_frames(frames, str(tmp_path), 1, 0, False, boundary=str(tdir)) == [0, 1, 2]


# ---- GPU ------------------------------------------------------------------------------------------------

def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _u64(t):
    import torch

    return t.view(torch.int64).cpu().numpy().astype(np.uint64)


@pytest.mark.gpu
def test_counts_equal_the_reference(gold, names, cuda):
    """Fails on the parent commit: dp_boundary_counts does not exist there."""
    from depth_pro.eval import boundary_metrics as M

    th = gold["thresholds"]
    th32 = th.astype(np.float32).astype(np.float64)
    for name in names:
        pred, tgt, alpha = _case(gold, name)
        p = _dev(pred, cuda)
        got = _u64(M.boundary_counts(p, _dev(tgt, cuda), th, M.DP_BOUNDARY_DEPTH))
        assert np.array_equal(got, gold[f"{name}_plain"]), (name, "depth", np.argwhere(got != gold[f"{name}_plain"])[:5].tolist())
        got = _u64(M.boundary_counts(p, _dev(alpha > 0.1, cuda), th32, M.DP_BOUNDARY_MASK))
        assert np.array_equal(got, gold[f"{name}_thin"]), (name, "mask", np.argwhere(got != gold[f"{name}_thin"])[:5].tolist())


@pytest.mark.gpu
def test_more_than_one_pass_of_thresholds(gold, cuda):
    """17 and 32 thresholds: the thinned walk keeps 16 per pass."""
    from depth_pro.eval import boundary_metrics as M

    pred, tgt, alpha = _case(gold, "scene")
    for n in (16, 17, 32):
        th = np.linspace(1.02, 1.6, n)
        got = _u64(M.boundary_counts(_dev(pred, cuda), _dev(alpha > 0.1, cuda), th, M.DP_BOUNDARY_MASK))
        assert np.array_equal(got, B.counts(B.invert_depth(pred), alpha > 0.1, th, "mask", "f64")), n
        got = _u64(M.boundary_counts(_dev(pred, cuda), _dev(tgt, cuda), th, M.DP_BOUNDARY_DEPTH))
        assert np.array_equal(got, B.counts(B.invert_depth(pred), B.invert_depth(tgt), th, "depth", "f64")), n


@pytest.mark.gpu
def test_edge_maps_equal_the_reference(gold, names, cuda):
    from depth_pro.eval import boundary_metrics as M

    th = gold["thresholds"]
    for name in names:
        pred = gold[f"{name}_pred"]
        p = _dev(pred, cuda)
        for k in gold["map_k"]:
            got = M.boundary_edges(p, th[k]).cpu().numpy()
            want = _maps(gold, name, "pmap", k)
            assert np.array_equal(got, want), (name, k, "plain", int((got != want).sum()))
            got = M.boundary_edges(p, float(np.float32(th[k])), thinned=True).cpu().numpy()
            want = _maps(gold, name, "tmap", k)
            assert np.array_equal(got, want), (name, k, "thinned", np.argwhere(got != want)[:5].tolist())
            assert not got[0, :, -1].any() and not got[2, :, -1].any() and not got[1, -1].any() and not got[3, -1].any()


@pytest.mark.gpu
def test_scores_equal_the_reference(gold, names, cuda):
    from depth_pro.eval import boundary_metrics as M

    for name in names:
        pred, tgt, alpha = _case(gold, name)
        _same_score(M.SI_boundary_F1(_dev(pred, cuda), _dev(tgt, cuda)), float(gold[f"{name}_f1"]), gold)
        _same_score(M.SI_boundary_Recall(_dev(pred, cuda), _dev(alpha, cuda)), float(gold[f"{name}_recall"]), gold)
    pred, tgt, alpha = _case(gold, "scene")
    th = gold["thresholds"]
    pi, gi, m = B.invert_depth(pred), B.invert_depth(tgt), alpha > 0.1
    for k in (0, 1, 9):          # the reference's single-threshold calls take inverse depths
        c = gold["scene_plain"][k].astype(np.int64).tolist()
        assert M.boundary_f1(pi, gi, th[k]) == M.f1_from_counts(c) and M.boundary_f1(pi, gi, th[k], return_p=True) == M.precision_from_counts(c)
        assert M.boundary_f1(_dev(pi, cuda), _dev(gi, cuda), th[k], return_r=True) == M.recall_from_counts(c)
        assert M.edge_recall_matting(pi, m, float(th[k])) == M.recall_from_counts(gold["scene_thin"][k].astype(np.int64).tolist())
    # masks as bool, uint8 (raw values) and float32 alpha
    want = float(gold["scene_recall"])
    _same_score(M.SI_boundary_Recall(pred, m), want, gold)
    _same_score(M.SI_boundary_Recall(_dev(pred, cuda), _dev(m.astype(np.uint8) * 200, cuda)), want, gold)


@pytest.mark.gpu
def test_strided_numpy_and_repeated_calls(gold, cuda):
    import torch

    from depth_pro.eval import boundary_metrics as M

    pred, tgt, alpha = _case(gold, "scene")
    th = gold["thresholds"]
    h, w = pred.shape
    wide = torch.full((h, w + 13), float("nan"), device=cuda)
    wide[:, :w] = _dev(pred, cuda)
    wide_t = torch.full((h, w + 5), 7.0, device=cuda)
    wide_t[:, :w] = _dev(tgt, cuda)
    wide_m = torch.ones((h, w + 3), dtype=torch.uint8, device=cuda)
    wide_m[:, :w] = _dev((alpha > 0.1).astype(np.uint8), cuda)
    pv, tv, mv = wide[:, :w], wide_t[:, :w], wide_m[:, :w]
    assert not pv.is_contiguous() and pv.stride(0) == w + 13
    a = M.boundary_counts(pv, tv, th, M.DP_BOUNDARY_DEPTH)
    b = M.boundary_counts(pv, mv, th, M.DP_BOUNDARY_MASK)
    assert np.array_equal(_u64(a), gold["scene_plain"])
    assert np.array_equal(_u64(b), B.counts(B.invert_depth(pred), alpha > 0.1, th, "mask", "f64"))
    assert np.array_equal(_u64(M.boundary_counts(pred, tgt, th, M.DP_BOUNDARY_DEPTH)), gold["scene_plain"])          # numpy in
    assert np.array_equal(_u64(M.boundary_counts(pred, alpha > 0.1, th, M.DP_BOUNDARY_MASK)), _u64(b))
    e1 = M.boundary_edges(pv, th[3], thinned=True)
    assert torch.equal(e1, M.boundary_edges(_dev(pred, cuda), th[3], thinned=True))
    for _ in range(2):           # two calls give identical bytes
        assert torch.equal(M.boundary_counts(pv, tv, th, M.DP_BOUNDARY_DEPTH).view(torch.int64), a.view(torch.int64))
        assert torch.equal(M.boundary_counts(pv, mv, th, M.DP_BOUNDARY_MASK).view(torch.int64), b.view(torch.int64))
        assert torch.equal(M.boundary_edges(pv, th[3], thinned=True), e1)


@pytest.mark.gpu
def test_argument_error_leaves_counts_untouched(gold, cuda):
    import torch

    from depth_pro import _lib

    lib = _lib.load()
    p = _dev(gold["scene_pred"], cuda)
    h, w = p.shape
    out = torch.full((10, 4, 3), 77, dtype=torch.int64, device=cuda)
    ws = torch.empty(int(lib.dp_boundary_workspace_size(h, w, 10)), dtype=torch.uint8, device=cuda)
    th = (ctypes.c_double * 10)(*gold["thresholds"])
    stream = torch.cuda.current_stream().cuda_stream
    bad = (ctypes.c_double * 10)(*([1.1] * 9 + [float("nan")]))
    assert lib.dp_boundary_counts(p.data_ptr(), w, p.data_ptr(), w, 0, h, w, bad, 10, out.data_ptr(), ws.data_ptr(), ws.numel(), stream) == ARG
    assert lib.dp_boundary_counts(p.data_ptr(), w - 1, p.data_ptr(), w, 0, h, w, th, 10, out.data_ptr(), ws.data_ptr(), ws.numel(), stream) == SHAPE
    assert lib.dp_boundary_counts(p.data_ptr(), w, p.data_ptr(), w, 1, h, w, th, 10, out.data_ptr(), ws.data_ptr(), ws.numel() - 1, stream) == ARG
    torch.cuda.synchronize()
    assert (out == 77).all().item()
    assert lib.dp_boundary_counts(p.data_ptr(), w, p.data_ptr(), w, 0, h, w, th, 10, out.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got == gold["scene_plain"][:, :, 2:3].astype(np.int64)).all()          # prediction against itself: all three counts


@pytest.mark.gpu
def test_generate_depth_maps_boundary(tmp_path, gold, cuda, capsys):
    """--boundary_dir on two tiny frames with synthetic depths: one depth target, one mask target; the JSONs hold counts that
    re-score to the stored score, and the score is the reference's for the depth the loop wrote."""
    import torch
    from PIL import Image

    import generate_depth_maps as G
    from depth_pro.eval import boundary_metrics as M

    pred, tgt, alpha = _case(gold, "scene")
    h, w = pred.shape
    src, out, tdir = tmp_path / "frames", tmp_path / "out", tmp_path / "targets"
    src.mkdir()
    tdir.mkdir()
    for k in range(3):
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(src / f"output_{k:04d}.png")
    np.save(tdir / "output_0000.npy", tgt)
    np.save(tdir / "output_0001.npy", (alpha * 255).astype(np.uint8))          # raw values, thresholded by > 0.1
    np.save(tdir / "output_0002.npy", tgt[:-1])                                # mis-shaped: reported and skipped

    class Model:
        def infer(self, x, f_px=None):
            return {"depth": _dev(pred, cuda).clone(), "focallength_px": torch.tensor(100.0, device=cuda)}

    kw = dict(pattern="output_*.png", model=(Model(), lambda im: torch.as_tensor(np.asarray(im))), boundary_dir=str(tdir))
    assert G.batch_generate_depth_maps(str(src), str(out), **kw) == 3
    assert sorted(os.listdir(out)) == ["output_0000_boundary.json", "output_0000_depth.png", "output_0001_boundary.json",
                                       "output_0001_depth.png", "output_0002_depth.png"]
    text = capsys.readouterr().out
    assert "output_0002" in text and "mean boundary score over 2 frames" in text
    want = {"output_0000": ("depth", float(gold["scene_f1"]), M.DP_BOUNDARY_DEPTH),
            "output_0001": ("mask", B.si_boundary_recall(pred, (alpha * 255).astype(np.uint8)), M.DP_BOUNDARY_MASK)}
    for stem, (kind, score, code) in want.items():
        js = json.load(open(out / f"{stem}_boundary.json"))
        assert js["kind"] == kind and (js["H"], js["W"]) == (h, w) and js["thresholds"] == list(gold["thresholds"])
        assert np.array(js["counts"]).shape == (10, 4, 3)
        assert M.weighted_score(js["counts"], js["thresholds"], code) == js["score"]
        _same_score(js["score"], score, gold)
    frames = sorted(str(p) for p in src.iterdir())
    assert G.plan_frames(frames, str(out), 1, 0, True, boundary=str(tdir)) == [2]      # a target without a JSON: not done
