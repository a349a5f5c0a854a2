"""Golden vectors for the boundary metric, from the REFERENCE's own functions.

Run where the reference checkout is at hand:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_boundary.py /path/to/reference
(or DEPTH_PRO_REFERENCE=/path/to/reference).  The reference's src/depth_pro/eval/boundary_metrics.py is imported from
its file at run time (it needs numpy only); no reference text is stored.  Output: golden_boundary.npz -- per case the
inputs (prediction, target depth, alpha mask, all float32) and what the reference returns for them:
  plain   [10, 4, 3]  both / target / predicted counts of fgbg_depth on both inverse depths (t an np.float64, as in boundary_f1)
  thin    [10, 4, 3]  the same with fgbg_depth_thinned(prediction, float(t)) and fgbg_binary_mask(alpha > 0.1)
  pmap_k, tmap_k      bit-packed uint8 [4, H, W] maps of fgbg_depth / fgbg_depth_thinned of the prediction, thresholds MAP_K
  f1, recall          SI_boundary_F1 / SI_boundary_Recall
and the numpy version as a string.  Thresholds: the default linspace(1.05, 1.25, 10).

The cases (SEG = 64, the kernels' segment length; a map's lines are W - 1 or H - 1 cells long):
  deg_*     1x1, 1x2, 2x1, 1x70, 70x1
  run_*     37x64, 37x65, 37x66, 3x257, 4x129, 4x130 and their transposes: rows with runs that end on, start on and
            straddle every multiple of 64 (asserted), growth factors between the thresholds so that a run splits as
            the threshold rises; the transposes put the same runs into columns
  whole_*   5x66 and 66x5: every cell of every row in one run (asserted: 5 runs per threshold, not 1)
  ties_*    6x150 and 150x6: the inverse depth doubles for 20 cells and restarts; every "right" ratio in a run is
            exactly 2 (asserted), so the first cell stays; the "left" map has lone cells of 2^20
  special   NaN inside a run, two +inf depths (an inf and a NaN ratio), 0 / negative / 1e-7 depths (all clipped),
            3e38 and 2e38 side by side (denormal inverse depths with the ratio 1.5); asserted ratio by ratio
  width     a pair whose fp32 ratio equals np.float32(t) > t for t = linspace(1.05, 1.25, 10)[1], found by searching
            the neighbouring float32 depths (asserted); the reference's F1 path counts the edge, its recall path
            does not (asserted)
  scene     97x131 boxes over a sloped floor (boundary_numpy.scene); 0 < F1 < 1, 0 < recall < 1 and every one of
            the 4 x 10 both / target / predicted counts of both kinds is non-zero (asserted)
and the generator asserts that tests/boundary_numpy.py reproduces every count, map and score.
"""

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import boundary_numpy as B  # noqa: E402

SEG = 64
MAP_K = (1, 7)
TH = np.linspace(1.05, 1.25, 10)


def reference():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DEPTH_PRO_REFERENCE")
    if not root:
        sys.exit("usage: make_golden_boundary.py /path/to/reference")
    path = os.path.join(root, "src", "depth_pro", "eval", "boundary_metrics.py")
    spec = importlib.util.spec_from_file_location("reference_boundary_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_rows(h, w, seed):
    """Rows whose "right" runs end on, start on and straddle every multiple of SEG.  Returns (depth, runs): per row
    the list of (first, last) cells of the runs at the lowest threshold."""
    rng = np.random.default_rng(seed)
    n = w - 1
    grow = np.array([1.07, 1.12, 1.18, 1.23, 1.3, 1.45])
    inv = np.ones((h, w))
    runs = []
    for i in range(h):
        cells = np.zeros(n, bool)
        for j, b in enumerate(range(SEG, n + 1, SEG)):
            lo, hi = ((b - 4, b - 1), (b, b + 3), (b - 3, b + 2))[(i + j) % 3]
            cells[max(lo, 0):min(hi, n - 1) + 1] = True
        for c in np.flatnonzero(rng.random(n) < 0.08):
            if not cells[max(c - 1, 0):c + 4].any():
                cells[c:c + int(rng.integers(1, 4))] = True
        f = rng.choice(grow, n)
        line = [1.0]
        for c in range(n):          # inside a run the inverse depth grows; outside it is 1 within 1 % (after a run: a "left" edge)
            line.append(line[-1] * f[c] if cells[c] else rng.uniform(0.99, 1.01))
        inv[i] = line
        edges = np.flatnonzero(np.diff(np.concatenate([[0], cells.astype(int), [0]])))
        runs.append(list(zip(edges[::2], edges[1::2] - 1)))
    return (4.0 / inv).astype(np.float32), runs


def mask_for(shape, seed):
    rng = np.random.default_rng(seed + 1000)
    return rng.choice(np.array([0, 0.05, 0.1, 0.15, 1], np.float32), shape)


def cases():
    out = {}
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (1, 2), (2, 1), (1, 70), (70, 1)):
        d = (2.0 * np.cumprod(rng.choice([0.8, 1.0, 1.3], h * w))).astype(np.float32).reshape(h, w)
        out[f"deg_{h}x{w}"] = (d, (d * rng.uniform(0.98, 1.02, d.shape)).astype(np.float32), mask_for(d.shape, h * w))
    for s, (h, w) in enumerate(((37, 64), (37, 65), (37, 66), (3, 257), (4, 129), (4, 130))):
        d, runs = run_rows(h, w, s)
        flat = [r for row in runs for r in row]
        for b in range(SEG, w, SEG):                              # w - 1 cells: 0 .. w - 2
            assert any(hi == b - 1 for lo, hi in flat), (h, w, b)
            if b <= w - 2:
                assert any(lo == b for lo, hi in flat) and any(lo < b <= hi for lo, hi in flat), (h, w, b)
        tgt = (d * np.random.default_rng(s).uniform(0.98, 1.02, d.shape)).astype(np.float32)
        m = mask_for(d.shape, s)
        out[f"run_{h}x{w}"] = (d, tgt, m)
        out[f"run_{w}x{h}"] = (np.ascontiguousarray(d.T), np.ascontiguousarray(tgt.T), np.ascontiguousarray(m.T))
    inv = np.cumprod(np.random.default_rng(9).uniform(1.3, 1.5, (5, 66)), axis=1)
    d = (1e6 / inv).astype(np.float32)
    assert d.min() > 1e-5
    m = mask_for(d.shape, 9)
    out["whole_5x66"] = (d, d.copy(), m)
    out["whole_66x5"] = (np.ascontiguousarray(d.T), np.ascontiguousarray(d.T), np.ascontiguousarray(m.T))
    y, x = np.mgrid[0:6, 0:150]
    d = (1024.0 * 2.0 ** -((x + 3 * y) % 21)).astype(np.float32)
    m = mask_for(d.shape, 11)
    out["ties_6x150"] = (d, np.roll(d, 2, axis=1), m)
    out["ties_150x6"] = (np.ascontiguousarray(d.T), np.ascontiguousarray(np.roll(d, 2, axis=1).T), np.ascontiguousarray(m.T))
    d = np.full((8, 40), 2.0, np.float32)
    d[0, :12] = 2.0 / 1.3 ** np.arange(12)
    d[0, 6] = np.nan                                  # a NaN inside a run of "right" edges
    d[1, 5:7] = np.inf                                # inf, inf: x / 0 = inf, 0 / 0 = NaN, 0 / x = 0
    d[2, 3], d[2, 4], d[2, 5], d[2, 6] = 0.0, -3.0, 1e-7, -np.inf      # all clipped to 1e-6
    d[3, 10:12] = [3e38, 2e38]                        # both inverse depths are float32 denormals; their ratio is 1.5
    d[4, 8:11] = np.inf                               # inf, inf, inf in a row: NaN ratios between them
    d[5, 20:23] = [np.inf, 1.0, np.inf]
    d[6, 2:6] = [np.inf, 2.0, 1.0, np.inf]            # right ratios: inf, 2, 0 -> one run, the inf first
    d[6, 12:17] = [1.0, 0.5, np.inf, 7.0, np.inf]
    d[7, 30:34] = [np.inf, 4.0, 2.0, 1.0]             # right: inf, 2, 2: the inf stays
    d[7, 1:5] = [1.0, np.inf, np.inf, 1.0]
    out["special"] = (d, np.ascontiguousarray(d[::-1]), mask_for(d.shape, 13))
    out["special_t"] = (np.ascontiguousarray(d.T), np.ascontiguousarray(d[::-1].T), np.ascontiguousarray(mask_for(d.shape, 13).T))
    out["width"] = width_case()
    out["scene"] = B.scene(97, 131, 3)
    return out


def width_case():
    t = TH[1]
    t32 = np.float32(t)
    assert float(t32) > t
    for db in np.float32([1.0, 2.0, 3.0, 1.5, 5.0, 0.7]):
        ib = np.float32(1.0) / db
        guess = np.float32(1.0 / (float(ib) * t))
        cand = guess
        for _ in range(200):
            cand = np.nextafter(cand, np.float32(0))
        for _ in range(400):
            if (np.float32(1.0) / cand) / ib == t32:
                d = np.full((3, 4), db, np.float32)
                d[1, 1] = cand                                     # left of (1, 1)-(1, 2) and right of (1, 0)-(1, 1) equal t32
                return d, d.copy(), np.zeros((3, 4), np.float32)
            cand = np.nextafter(cand, np.float32(np.inf))
    raise AssertionError("no pair with ratio == float32(t)")


def main():
    ref = reference()
    save = {"numpy_version": np.str_(np.__version__), "thresholds": TH, "map_k": np.array(MAP_K),
            "names": np.array(list(cases().keys()))}
    for name, (pred, tgt, alpha) in cases().items():
        assert pred.dtype == tgt.dtype == alpha.dtype == np.float32 and pred.shape == tgt.shape == alpha.shape
        with np.errstate(all="ignore"):
            pi, gi, m = ref.invert_depth(pred), ref.invert_depth(tgt), alpha > 0.1
            assert pi.dtype == np.float32
            plain, thin = np.zeros((10, 4, 3), np.uint64), np.zeros((10, 4, 3), np.uint64)
            for k, t in enumerate(TH):
                p, g = ref.fgbg_depth(pi, t), ref.fgbg_depth(gi, t)
                pt, gm = ref.fgbg_depth_thinned(pi, float(t)), ref.fgbg_binary_mask(m)
                for d in range(4):
                    plain[k, d] = (np.count_nonzero(p[d] & g[d]), np.count_nonzero(g[d]), np.count_nonzero(p[d]))
                    thin[k, d] = (np.count_nonzero(pt[d] & gm[d]), np.count_nonzero(gm[d]), np.count_nonzero(pt[d]))
                if k in MAP_K:
                    save[f"{name}_pmap_{k}"] = np.packbits(B.padded(p, pred.shape))
                    save[f"{name}_tmap_{k}"] = np.packbits(B.padded(pt, pred.shape))
                    assert np.array_equal(B.padded(B.plain_edges(B.invert_depth(pred), t, "f64"), pred.shape), B.padded(p, pred.shape)), name
                    assert np.array_equal(B.padded(B.thinned_edges(B.invert_depth(pred), t, "f32"), pred.shape), B.padded(pt, pred.shape)), name
            f1, rec = ref.SI_boundary_F1(pred, tgt), ref.SI_boundary_Recall(pred, alpha)
        save.update({f"{name}_pred": pred, f"{name}_target": tgt, f"{name}_alpha": alpha, f"{name}_plain": plain,
                     f"{name}_thin": thin, f"{name}_f1": np.float64(f1), f"{name}_recall": np.float64(rec)})
        assert np.array_equal(B.counts(B.invert_depth(pred), B.invert_depth(tgt), TH, "depth", "f64"), plain), name
        assert np.array_equal(B.counts(B.invert_depth(pred), m, TH, "mask", "f32"), thin), name
        assert B.si_boundary_f1(pred, tgt) == f1 and B.si_boundary_recall(pred, alpha) == rec, name
        print(f"{name:12s} {str(pred.shape):10s} f1 {f1:.6f} recall {rec:.6f} plain pred {plain[:, :, 2].sum()} thin pred {thin[:, :, 2].sum()}")
        checks(name, ref, pred, pi, plain, thin, f1, rec)
    np.savez_compressed(os.path.join(HERE, "golden_boundary.npz"), **save)
    print("golden_boundary.npz", os.path.getsize(os.path.join(HERE, "golden_boundary.npz")), "bytes")


def checks(name, ref, pred, pi, plain, thin, f1, rec):
    if name.startswith("deg_1x1"):
        assert not plain.any() and not thin.any() and f1 == 0.0 and rec == 0.0
    if name == "whole_5x66":
        assert (thin[:, 2, 2] == 5).all() and (plain[:, 2, 2] == 5 * 65).all()
    if name == "whole_66x5":
        assert (thin[:, 3, 2] == 5).all() and (plain[:, 3, 2] == 5 * 65).all()
    if name == "ties_6x150":
        with np.errstate(all="ignore"):
            l, _, r, _ = B.ratios(pi)
        assert set(np.unique(r)) == {np.float32(2.0), np.float32(2.0 ** -20)} and l.max() == 2.0 ** 20
        kept = ref.fgbg_depth_thinned(pi, float(TH[3]))[2]
        run = r == 2.0
        first = run & ~np.pad(run, ((0, 0), (1, 0)))[:, :-1]
        assert np.array_equal(kept, first) and (thin[:, 0, 2] == (l == 2.0 ** 20).sum()).all()
    if name == "special":
        with np.errstate(all="ignore"):
            l, _, r, _ = B.ratios(pi)
        assert np.isnan(r[0, 5]) and np.isnan(r[0, 6]) and r[0, 4] > 1.29 and r[0, 7] > 1.29        # the NaN splits the run
        assert np.isnan(r[1, 5]) and np.isinf(l[1, 4]) and r[1, 4] == 0 and np.isinf(r[1, 6])
        assert (pi[2, 3:7] == np.float32(1e6)).all() and (r[2, 3:6] == 1).all()
        tiny = np.finfo(np.float32).tiny
        assert 0 < pi[3, 10] < pi[3, 11] < tiny and np.isfinite(l[3, 9]) and l[3, 9] > 1e37 and 1.49 < r[3, 10] < 1.51
        assert np.isnan(r[4, 8]) and np.isnan(r[4, 9])
        assert np.isinf(r[6, 2]) and r[6, 3] == 2 and r[6, 4] == 0
        kept = ref.fgbg_depth_thinned(pi, float(TH[0]))[2]
        assert kept[6, 2] and not kept[6, 3] and kept[7, 30] and not kept[7, 31] and not kept[7, 32]
        assert kept[0, :5].sum() == 1 and kept[0, 7:11].sum() == 1
    if name == "width":
        t = TH[1]
        l = B.ratios(pi)[0]
        assert l[1, 1] == np.float32(t) and float(l[1, 1]) > t
        assert ref.fgbg_depth(pi, t)[0][1, 1] and not ref.fgbg_depth_thinned(pi, float(t))[0][1, 1]
        assert plain[1, 0, 2] == 1 and thin[1, 0, 2] == 0 and plain[0, 0, 2] == 1 and thin[0, 0, 2] == 1
    if name == "scene":
        assert 0 < f1 < 1 and 0 < rec < 1 and (plain > 0).all() and (thin > 0).all()


if __name__ == "__main__":
    main()
