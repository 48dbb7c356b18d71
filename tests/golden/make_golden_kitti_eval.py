#!/usr/bin/env python
"""Golden fixture for the KITTI evaluator (ws3d_amd/kitti_eval.py), produced by running the REFERENCE's own
tools/kitti_object_eval_python/{eval,rotate_iou,kitti_common}.py on a synthetic 64-frame label / result set:
``python -B tests/golden/make_golden_kitti_eval.py``.

Runs only in the build container (imports /root/reference).  numba, numba.cuda and skimage are not installed:
stand-in modules defined below make ``jit`` the identity and ``cuda.local.array`` a float32 numpy array, so the
reference's functions run as plain Python.  Its numba.cuda kernel launch (rotate_iou_gpu_eval) is replaced by a
Python double loop over the reference's own ``devRotateIoUEval``; pairs whose centres are farther apart than the
sum of the half-diagonals are skipped (they have no intersection point, so the reference's value is 0 as well).

Written: tests/golden/kitti_eval.npz (the label / result texts, the per-frame overlap blocks of metrics 0 / 1 / 2,
a dense pair set under criteria -1 / 0 / 1 / 2, counting-mode pr arrays, eval_class arrays) and
tests/golden/kitti_eval.json (get_official_eval_result's string and dict per class selection, the parsed
annotations of a few files).  Data only.
"""
from __future__ import annotations

import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

import numpy as np  # noqa: E402

FRAMES = 64
SEED = 20261016
THRESH = (0.25, 0.5, 0.7)
BIG_DT_FRAME, BIG_GT_FRAME = 5, 17           # > 64 detections / > 64 ground truths
EMPTY_FRAMES = {9: "neither", 10: "no_dt", 11: "no_gt", 40: "no_gt"}
COUNT_THRESHOLDS = np.array([-1.0, 0.123455, 0.345675, 0.5, 0.654325, 0.876545, 0.987655, 2.0])
CLASS_SELECTIONS = {"0": 0, "1": 1, "2": 2, "012": [0, 1, 2]}


def install_stubs():
    numba = types.ModuleType("numba")

    def jit(*args, **kw):
        if len(args) == 1 and callable(args[0]) and not kw:
            return args[0]
        return lambda f: f

    cuda = types.ModuleType("numba.cuda")
    cuda.jit = jit
    cuda.local = types.SimpleNamespace(array=lambda shape, dtype=None: np.zeros(shape, np.float32))
    cuda.shared = cuda.local
    numba.jit = jit
    numba.njit = jit
    numba.float32 = np.float32
    numba.cuda = cuda
    sys.modules["numba"] = numba
    sys.modules["numba.cuda"] = cuda
    sk = types.ModuleType("skimage")
    sk.io = types.ModuleType("skimage.io")
    sys.modules["skimage"] = sk
    sys.modules["skimage.io"] = sk.io
    sys.modules.setdefault("fire", types.ModuleType("fire"))


def import_reference():
    install_stubs()
    sys.path.insert(0, REF)
    import tools.kitti_object_eval_python.rotate_iou as ri
    import tools.kitti_object_eval_python.eval as ev
    import tools.kitti_object_eval_python.kitti_common as kc

    def rotate_iou_loop(boxes, query_boxes, criterion=-1, device_id=0):
        b = boxes.astype(np.float32)
        q = query_boxes.astype(np.float32)
        iou = np.zeros((b.shape[0], q.shape[0]), dtype=np.float32)
        if iou.size == 0:
            return iou
        rb = 0.5 * np.sqrt(b[:, 2].astype(np.float64) ** 2 + b[:, 3].astype(np.float64) ** 2)
        rq = 0.5 * np.sqrt(q[:, 2].astype(np.float64) ** 2 + q[:, 3].astype(np.float64) ** 2)
        d2 = (b[:, None, 0].astype(np.float64) - q[None, :, 0]) ** 2 + (b[:, None, 1].astype(np.float64) - q[None, :, 1]) ** 2
        near = d2 <= (rb[:, None] + rq[None, :]) ** 2 * 1.0001 + 1e-6
        for n, k in zip(*np.nonzero(near)):
            iou[n, k] = ri.devRotateIoUEval(q[k].copy(), b[n].copy(), criterion)
        return iou

    ev.rotate_iou_gpu_eval = rotate_iou_loop
    return ev, kc, rotate_iou_loop


# ----------------------------------------------------------------------------- scene
DIMS = {"Car": (1.5, 1.6, 3.9), "Van": (2.1, 1.9, 5.0), "Pedestrian": (1.75, 0.6, 0.8), "Cyclist": (1.7, 0.6, 1.8),
        "Person_sitting": (1.2, 0.6, 0.8), "Truck": (3.2, 2.5, 10.0)}
GT_CLASSES = ["Car", "Car", "Car", "Car", "Van", "Pedestrian", "Pedestrian", "Cyclist", "Cyclist", "Person_sitting", "Truck", "DontCare"]
DT_CLASSES = ["Car", "Car", "Car", "Pedestrian", "Cyclist"]


def _ry(rng):
    if rng.uniform() < 0.2:     # near +-pi
        return float(np.pi * rng.choice([-1, 1]) - rng.choice([-1, 1]) * rng.uniform(0, 0.05))
    return float(rng.uniform(-np.pi, np.pi))


def make_frame(rng, f):
    kind = EMPTY_FRAMES.get(f)
    n_gt = 0 if kind in ("neither", "no_gt") else (72 if f == BIG_GT_FRAME else int(rng.integers(1, 11)))
    slots = rng.permutation([(x, z) for x in range(-24, 25, 6) for z in range(6, 66, 6)])[:n_gt]
    gts = []
    for x, z in slots:
        cls = str(rng.choice(GT_CLASSES))
        if cls == "DontCare":
            l0 = float(rng.uniform(0, 1100)); t0 = float(rng.uniform(100, 250))
            gts.append(dict(name=cls, trunc=-1, occ=-1, alpha=-10, bbox=(l0, t0, l0 + rng.uniform(20, 200), t0 + rng.uniform(10, 80)),
                            hwl=(-1, -1, -1), loc=(-1000, -1000, -1000), ry=-10))
            continue
        h, w, l = DIMS[cls]
        h, w, l = h * rng.uniform(0.9, 1.1), w * rng.uniform(0.9, 1.1), l * rng.uniform(0.9, 1.1)
        height = float(rng.choice([18, 24, 30, 38, 45, 60, 90, 130]) + rng.uniform(-2, 2))
        width = height * rng.uniform(0.5, 2.0)
        l0 = float(rng.uniform(0, 1200 - width)); t0 = float(rng.uniform(100, 370 - height))
        gts.append(dict(name=cls, trunc=float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6])), occ=int(rng.choice([0, 0, 1, 2, 3])),
                        alpha=float(rng.uniform(-np.pi, np.pi)), bbox=(l0, t0, l0 + width, t0 + height), hwl=(h, w, l),
                        loc=(x + rng.uniform(-0.5, 0.5), rng.uniform(1.0, 2.0), z + rng.uniform(-0.5, 0.5)), ry=_ry(rng)))
    dts = []
    if kind not in ("neither", "no_dt"):
        target = 80 if f == BIG_DT_FRAME else None
        real = [g for g in gts if g["name"] != "DontCare"]
        for g in real:
            for _ in range(int(rng.choice([0, 1, 1, 1, 2]))):
                mode = rng.choice(["copy", "jit_s", "jit_m", "jit_l", "dup"])
                s = {"copy": 0.0, "dup": 0.0, "jit_s": 0.08, "jit_m": 0.25, "jit_l": 0.5}[str(mode)]
                loc = tuple(np.array(g["loc"]) + rng.normal(0, s, 3) * np.array([g["hwl"][2], 0.3, g["hwl"][2]]))
                hwl = tuple(np.array(g["hwl"]) * (1 + rng.normal(0, s / 2, 3)))
                bb = np.array(g["bbox"]) + rng.normal(0, s * 20, 4)
                if rng.uniform() < 0.1:
                    bb[3] = bb[1] + rng.choice([20.0, 33.0])          # shorter than 25 / 40 px
                ry = g["ry"] + rng.normal(0, s)
                name = g["name"] if g["name"] in ("Car", "Pedestrian", "Cyclist") and rng.uniform() < 0.85 else str(rng.choice(DT_CLASSES))
                dts.append(dict(name=name, alpha=g["alpha"] + rng.normal(0, 0.3), bbox=tuple(bb), hwl=hwl, loc=loc, ry=float(ry)))
                if mode == "dup":
                    dts.append(dict(dts[-1]))
        n_fp = int(rng.integers(0, 6)) if target is None else max(0, target - len(dts))
        for _ in range(n_fp):
            cls = str(rng.choice(DT_CLASSES))
            h, w, l = DIMS[cls]
            height = float(rng.uniform(15, 120)); width = height * rng.uniform(0.5, 2.0)
            l0 = float(rng.uniform(0, 1200 - width)); t0 = float(rng.uniform(100, 370 - height))
            dts.append(dict(name=cls, alpha=float(rng.uniform(-np.pi, np.pi)), bbox=(l0, t0, l0 + width, t0 + height), hwl=(h, w, l),
                            loc=(rng.uniform(-25, 25), rng.uniform(1, 2), rng.uniform(5, 65)), ry=_ry(rng)))
    tie_scores = [0.5, 0.75, 0.9]
    for d in dts:
        d["score"] = float(rng.choice(tie_scores)) if rng.uniform() < 0.15 else float(rng.uniform(0.05, 1.0))
    return gts, dts


def label_text(gts):
    return "".join("%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n" %
                   (g["name"], g["trunc"], g["occ"], g["alpha"], *g["bbox"], *g["hwl"], *g["loc"], g["ry"]) for g in gts)


def result_text(dts):
    return "".join("%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f\n" %
                   (d["name"], d["alpha"], *d["bbox"], *d["hwl"], *d["loc"], d["ry"], d["score"]) for d in dts)


def _anno_from_text(kc, text, tmp):
    p = os.path.join(tmp, "000000.txt")
    with open(p, "w") as f:
        f.write(text)
    return kc.get_label_anno(p)


def frame_is_safe(ev, gt, dt):
    """no overlap of any metric within 1e-4 of a min_overlap (fp32 rounding cannot flip a match)"""
    vals = []
    for metric in (0, 1, 2):
        vals.append(ev.calculate_iou_partly([dt], [gt], metric, 1)[0][0].ravel())
    dc = gt["bbox"][gt["name"] == "DontCare"]
    if len(dc) and len(dt["bbox"]):
        vals.append(ev.image_box_overlap(dt["bbox"], dc, 0).ravel())
    v = np.concatenate(vals) if vals else np.zeros(0)
    return not any(np.any(np.abs(v - t) < 1e-4) for t in THRESH)


def pack_texts(texts):
    b = [t.encode() for t in texts]
    off = np.zeros(len(b) + 1, np.int64)
    np.cumsum([len(x) for x in b], out=off[1:])
    return np.frombuffer(b"".join(b), dtype=np.uint8), off


def main():
    import tempfile
    ev, kc, rot = import_reference()
    rng = np.random.default_rng(SEED)
    tmp = tempfile.mkdtemp(prefix="ws3d_kitti_eval_")
    labels, results, gt_annos, dt_annos, redraws = [], [], [], [], 0
    for f in range(FRAMES):
        while True:
            gts, dts = make_frame(rng, f)
            lt, rt = label_text(gts), result_text(dts)
            gt, dt = _anno_from_text(kc, lt, tmp), _anno_from_text(kc, rt, tmp)
            if frame_is_safe(ev, gt, dt):
                break
            redraws += 1
        labels.append(lt); results.append(rt); gt_annos.append(gt); dt_annos.append(dt)
    assert sum(len(a["name"]) > 64 for a in dt_annos) >= 1 and sum(len(a["name"]) > 64 for a in gt_annos) >= 1

    out = {}
    out["label_bytes"], out["label_off"] = pack_texts(labels)
    out["result_bytes"], out["result_off"] = pack_texts(results)
    # per-frame (n_dt, n_gt) overlap blocks, as eval_class asks for them (calculate_iou_partly(dt_annos, gt_annos, ...))
    for metric in (0, 1, 2):
        blocks = ev.calculate_iou_partly(dt_annos, gt_annos, metric, 50)[0]
        flat = np.concatenate([b.ravel() for b in blocks])
        out[f"overlaps_m{metric}"] = flat if metric == 0 else flat.astype(np.float32)
    # dense pairs under the four criteria: boxes near one another, near +-pi, exact copies
    prng = np.random.default_rng(7)
    q = np.stack([prng.uniform(-3, 3, 20), prng.uniform(5, 11, 20), prng.uniform(1, 5, 20), prng.uniform(0.5, 2.5, 20),
                  prng.uniform(-np.pi, np.pi, 20)], 1)
    q[:4, 4] = [np.pi - 1e-3, -np.pi + 1e-3, np.pi, -np.pi]
    b = np.concatenate([q[:6] + prng.normal(0, 0.3, (6, 5)) * [1, 1, 0.2, 0.1, 0.2], q[6:10],
                        np.stack([prng.uniform(-4, 4, 14), prng.uniform(4, 12, 14), prng.uniform(1, 5, 14), prng.uniform(0.5, 2.5, 14),
                                  prng.uniform(-np.pi, np.pi, 14)], 1)])
    out["pair_boxes"], out["pair_query"] = b, q
    for c in (-1, 0, 1, 2):
        out[f"pair_c{c + 1}"] = rot(b, q, c)
    # counting-mode pr arrays at fixed thresholds: class 0, difficulty 1, each metric, both overlaps, with AOS
    for metric in (0, 1, 2):
        blocks = ev.calculate_iou_partly(dt_annos, gt_annos, metric, 50)[0]
        gt_n = np.array([len(a["name"]) for a in gt_annos]); dt_n = np.array([len(a["name"]) for a in dt_annos])
        full = np.zeros((dt_n.sum(), gt_n.sum()))
        go, do = np.concatenate([[0], np.cumsum(gt_n)]), np.concatenate([[0], np.cumsum(dt_n)])
        for i, blk in enumerate(blocks):
            full[do[i]:do[i + 1], go[i]:go[i + 1]] = blk
        (gt_datas, dt_datas, ignored_gts, ignored_dets, dontcares, dc_num, _) = ev._prepare_data(gt_annos, dt_annos, 0, 1)
        for k, mo in enumerate((0.7, 0.5)):
            pr = np.zeros([len(COUNT_THRESHOLDS), 4])
            ev.fused_compute_statistics(full, pr, gt_n, dt_n, dc_num, np.concatenate(gt_datas), np.concatenate(dt_datas),
                                        np.concatenate(dontcares), np.concatenate(ignored_gts), np.concatenate(ignored_dets), metric,
                                        min_overlap=mo, thresholds=COUNT_THRESHOLDS, compute_aos=True)
            out[f"pr_m{metric}_k{k}"] = pr
    out["count_thresholds"] = COUNT_THRESHOLDS
    # eval_class arrays and the official result per class selection
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25], [0.5, 0.25, 0.25, 0.5, 0.25]])
    js = {"generator": "tests/golden/make_golden_kitti_eval.py", "frames": FRAMES, "seed": SEED, "redraws": redraws, "official": {}}
    for key, sel in CLASS_SELECTIONS.items():
        cls = sel if isinstance(sel, list) else [sel]
        mo = np.stack([overlap_0_7, overlap_0_5], 0)[:, :, cls]
        for metric in (0, 1, 2):
            r = ev.eval_class(gt_annos, dt_annos, cls, [0, 1, 2], metric, mo, compute_aos=(metric == 0))
            for name in ("recall", "precision", "orientation"):
                out[f"ec_{key}_m{metric}_{name}"] = r[name]
        s, d = ev.get_official_eval_result(gt_annos, dt_annos, sel)
        js["official"][key] = {"result": s, "ret_dict": {k: float(v) for k, v in d.items()}}
        print(s)
    # parsed annotations of a few files (empty, big, DontCare-bearing, result with scores)
    js["annos"] = {}
    for f in (0, 9, BIG_GT_FRAME):
        js["annos"]["label_%d" % f] = {k: np.asarray(v).tolist() for k, v in gt_annos[f].items()}
        js["annos"]["label_%d_dtypes" % f] = {k: str(np.asarray(v).dtype) for k, v in gt_annos[f].items()}
    for f in (0, 9, BIG_DT_FRAME):
        js["annos"]["result_%d" % f] = {k: np.asarray(v).tolist() for k, v in dt_annos[f].items()}
        js["annos"]["result_%d_dtypes" % f] = {k: str(np.asarray(v).dtype) for k, v in dt_annos[f].items()}
    np.savez_compressed(os.path.join(HERE, "kitti_eval.npz"), **out)
    with open(os.path.join(HERE, "kitti_eval.json"), "w") as fh:
        json.dump(js, fh, indent=1)
    print("frames", FRAMES, "redraws", redraws, "gt", sum(len(a["name"]) for a in gt_annos), "dt", sum(len(a["name"]) for a in dt_annos))


if __name__ == "__main__":
    main()
