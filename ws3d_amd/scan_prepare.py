"""Scan preparation with a counter-based sampler: raw velodyne points -> ``pts_input``, on the device (csrc/scan_prepare.hip) or by the
bit-exact host restatement below (the CPU fallback and the reference of every test).

This is NOT the reference's sampler: ``kitti_io.rpn_input_from_scan`` reproduces that one (descending lidar-z sort, the global Mersenne
stream) and stays the default of every driver.  Here the draw is a function of ``(seed, scene_key)`` and the entry number alone, so raw
file order is the order and a scene's rows do not depend on the batch it travels in.  The contract (DESIGN.md "Scan preparation on the
device"), fp32 element-wise in exactly this order, no contraction, a NaN compares false::

    r_j   = ((x*T[0][j] + y*T[1][j]) + z*T[2][j]) + T[3][j]          T = V2C^T . R0^T (4 x 3), as Calibration.lidar_to_rect builds it
    h_k   = ((r_0*P[k][0] + r_1*P[k][1]) + r_2*P[k][2]) + P[k][3]    P = P2 (3 x 4)
    u = h_0 / r_2    v = h_1 / r_2    depth = h_2 - P[2][3]
    valid = u>=0 && u<W && v>=0 && v<H && depth>=0 && (scope: x0<=r_0<=x1 && y0<=r_1<=y1 && z0<=r_2<=z1)
    class = invalid | near (depth < 40) | far

    h(e) = splitmix64(splitmix64(seed + 0x9E3779B97F4A7C15 * scene_key) + e);  sel(e), ord(e) = the top key_bits of h's two halves

With V valid and F far points of n: V == 0 -> status 1; V > npoints and F > npoints -> status 2 (zero rows in both cases);
V > npoints -> every far point and the near points with the npoints - F smallest (sel(i), i), entry e = i; V <= npoints -> the entries
e = r n + i (r < ceil(npoints / V), i valid) with the npoints smallest (sel(e), e).  The kept entries are written ascending by
(ord(e), e); the row of entry e is [r_0, r_1, r_2, refl - 0.5] of point e mod n.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import kitti_io
from .kitti_io import PC_AREA_SCOPE

GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
INVALID, NEAR, FAR = 0, 1, 2
OK, EMPTY, TOO_FAR = 0, 1, 2            # status; the kernel adds 3 for device offsets that do not describe a slice
ROUTES = ("off", "device", "host")


def splitmix64(z) -> np.ndarray:
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = z + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def entry_keys(e: np.ndarray, seed: int, scene_key: int, key_bits: int = 32):
    """(sel, ord) of the entries e, both uint64 below 2**key_bits"""
    base = splitmix64((int(seed) + GOLDEN * (int(scene_key) & _M64)) & _M64)[0]
    with np.errstate(over="ignore"):
        h = splitmix64(base + np.asarray(e, dtype=np.uint64))
    shift = np.uint64(32 - key_bits)
    return (h >> np.uint64(32)) >> shift, (h & np.uint64(0xffffffff)) >> shift


def calib_tables(calib) -> np.ndarray:
    """(24,) float32: T (4 x 3), the right operand of ``Calibration.lidar_to_rect``, then P2 (3 x 4)"""
    T = np.dot(calib.V2C.T, calib.R0.T).astype(np.float32)
    return np.concatenate((T.reshape(-1), np.asarray(calib.P2, dtype=np.float32).reshape(-1)))


def project(raw: np.ndarray, tables: np.ndarray):
    """raw (n, >=3) float32 -> (rect (n,3), u, v, depth) by the contract's expressions"""
    raw = np.asarray(raw, dtype=np.float32)
    T, P = tables[:12].reshape(4, 3), tables[12:].reshape(3, 4)
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    with np.errstate(all="ignore"):
        r = [((x * T[0, j] + y * T[1, j]) + z * T[2, j]) + T[3, j] for j in range(3)]
        h = [((r[0] * P[k, 0] + r[1] * P[k, 1]) + r[2] * P[k, 2]) + P[k, 3] for k in range(3)]
        u, v, depth = h[0] / r[2], h[1] / r[2], h[2] - P[2, 3]
    return np.stack(r, axis=1), u, v, depth


def _scope6(area_scope):
    return None if area_scope is None else np.array([b for ax in area_scope for b in ax], dtype=np.float32)


def classify(raw: np.ndarray, tables: np.ndarray, img_shape, area_scope=PC_AREA_SCOPE):
    """-> (class (n,) uint8 of INVALID / NEAR / FAR, rect (n,3) float32)"""
    rect, u, v, depth = project(raw, tables)
    H, W = np.float32(img_shape[0]), np.float32(img_shape[1])
    with np.errstate(invalid="ignore"):
        valid = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth >= 0)
        s = _scope6(area_scope)
        if s is not None:
            valid &= ((rect[:, 0] >= s[0]) & (rect[:, 0] <= s[1]) & (rect[:, 1] >= s[2]) & (rect[:, 1] <= s[3])
                      & (rect[:, 2] >= s[4]) & (rect[:, 2] <= s[5]))
        cls = np.where(valid, np.where(depth < np.float32(40.0), NEAR, FAR), INVALID).astype(np.uint8)
    return cls, rect


def sample_entries(cls: np.ndarray, npoints: int, seed: int, scene_key: int, key_bits: int = 32):
    """the selection and order rules on a class vector -> (entries (npoints,) uint64 in output order, status); no entries unless status 0"""
    if npoints <= 0 or not 1 <= key_bits <= 32:
        raise ValueError(f"npoints={npoints} key_bits={key_bits}")
    n = len(cls)
    valid = np.flatnonzero(cls != INVALID).astype(np.uint64)
    far = np.flatnonzero(cls == FAR).astype(np.uint64)
    V, F = len(valid), len(far)
    if V == 0:
        return np.zeros(0, dtype=np.uint64), EMPTY
    if V > npoints and F > npoints:
        return np.zeros(0, dtype=np.uint64), TOO_FAR
    if V > npoints:
        cand, k, always = np.flatnonzero(cls == NEAR).astype(np.uint64), npoints - F, far
    else:
        reps = -(-npoints // V)
        cand = (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(n) + valid[None, :]).reshape(-1)
        k, always = npoints, np.zeros(0, dtype=np.uint64)
    sel, _ = entry_keys(cand, seed, scene_key, key_bits)
    kept = np.concatenate((always, cand[np.lexsort((cand, sel))[:k]]))
    _, order = entry_keys(kept, seed, scene_key, key_bits)
    return kept[np.lexsort((kept, order))], OK


def prepare_scans_host(scans: Sequence[np.ndarray], calibs, img_shapes, scene_keys, npoints: int = 16384, seed: int = 666,
                       area_scope=PC_AREA_SCOPE, key_bits: int = 32) -> dict:
    """the contract in numpy float32 / uint64 -> {'pts_input' (B,npoints,4) float32, 'src_index' (B,npoints) int32 (-1 in a failed
    scene), 'valid_count' (B,) int32, 'status' (B,) int32}.  calibs: ``kitti_io.Calibration`` objects (or (24,) tables)."""
    B = len(scans)
    out = {"pts_input": np.zeros((B, npoints, 4), dtype=np.float32), "src_index": np.full((B, npoints), -1, dtype=np.int32),
           "valid_count": np.zeros(B, dtype=np.int32), "status": np.zeros(B, dtype=np.int32)}
    for b, raw in enumerate(scans):
        raw = np.asarray(raw, dtype=np.float32).reshape(-1, 4)
        tables = calibs[b] if isinstance(calibs[b], np.ndarray) else calib_tables(calibs[b])
        cls, rect = classify(raw, tables, img_shapes[b], area_scope)
        entries, status = sample_entries(cls, npoints, seed, int(scene_keys[b]), key_bits)
        out["valid_count"][b], out["status"][b] = int((cls != INVALID).sum()), status
        if status == OK:
            i = (entries % np.uint64(len(raw))).astype(np.int64)
            out["pts_input"][b, :, 0:3] = rect[i]
            out["pts_input"][b, :, 3] = raw[i, 3] - np.float32(0.5)
            out["src_index"][b] = i
    return out


def _check_status(status: np.ndarray, valid_count: np.ndarray, scene_keys, npoints: int) -> None:
    for b in np.flatnonzero(status == TOO_FAR):
        raise ValueError(f"scene {scene_keys[b]}: more than npoints={npoints} of its {int(valid_count[b])} valid points lie beyond 40 m and do not fit")
    if (status > TOO_FAR).any():
        raise ValueError(f"scan offsets refused by the kernel (status {status.tolist()})")


def prepare_scans(scans: Sequence[np.ndarray], calibs, img_shapes, scene_keys, npoints: int = 16384, seed: int = 666,
                  area_scope=PC_AREA_SCOPE, key_bits: int = 32, device="cuda:0", check: bool = True) -> dict:
    """``prepare_scans_host``'s dict as tensors on `device`: the scans packed and uploaded, one ws3d_scan_prepare call on the current
    stream.  check: read the status back (one synchronisation) and raise ValueError for a scene whose far points do not fit, as the
    host route of the drivers does; check=False returns without reading anything back.  A CPU device, or sizes the kernel does not
    take (WS3D_E_UNSUPPORTED), go through the host restatement -- the same rows."""
    import torch
    dev = torch.device(device)
    if npoints <= 0 or not 1 <= key_bits <= 32:
        raise ValueError(f"npoints={npoints} key_bits={key_bits}")
    B = len(scans)
    if not (len(calibs) == len(img_shapes) == len(scene_keys) == B):
        raise ValueError("scans, calibs, img_shapes and scene_keys must have one entry per scene")

    def host():
        res = prepare_scans_host(scans, calibs, img_shapes, scene_keys, npoints, seed, area_scope, key_bits)
        if check:
            _check_status(res["status"], res["valid_count"], scene_keys, npoints)
        return {k: torch.from_numpy(v).to(dev) for k, v in res.items()}

    if dev.type != "cuda" or B == 0:
        return host()
    packed = pack_scans(scans, calibs, img_shapes, scene_keys)
    if packed["total"] > 0x7fffffff:
        return host()
    res = launch_packed(upload_packed(packed, dev), npoints, seed, area_scope, key_bits)
    if res is None:
        return host()
    if check:
        _check_status(res["status"].cpu().numpy(), res["valid_count"].cpu().numpy(), scene_keys, npoints)
    return res


def pack_scans(scans, calibs, img_shapes, scene_keys) -> dict:
    """the host arrays of one call: the scans back to back, their offsets, the calibration tables, image sizes and keys"""
    scans = [np.asarray(s, dtype=np.float32).reshape(-1, 4) for s in scans]
    offsets = np.zeros(len(scans) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in scans], out=offsets[1:])
    total = int(offsets[-1])
    return {"raw": np.concatenate(scans) if total else np.zeros((1, 4), dtype=np.float32), "offsets": offsets.astype(np.int32), "total": total,
            "max_n": max(len(s) for s in scans),
            "tables": np.stack([c if isinstance(c, np.ndarray) else calib_tables(c) for c in calibs]).astype(np.float32),
            "hw": np.array([[s[0], s[1]] for s in img_shapes], dtype=np.int32), "keys": np.array([int(k) for k in scene_keys], dtype=np.int64)}


def upload_packed(packed: dict, device) -> dict:
    import torch
    dev = torch.device(device)
    return {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in packed.items()}


def launch_packed(up: dict, npoints: int, seed: int = 666, area_scope=PC_AREA_SCOPE, key_bits: int = 32):
    """one ws3d_scan_prepare call on the current stream of the tensors' device -> the result dict, nothing read back; None when the
    kernel does not take the sizes (WS3D_E_UNSUPPORTED)"""
    import torch
    from . import _lib
    lib = _lib.load()
    dev, B = up["raw"].device, up["keys"].numel()
    with torch.cuda.device(dev):
        res = {"pts_input": torch.empty((B, npoints, 4), dtype=torch.float32, device=dev),
               "src_index": torch.empty((B, npoints), dtype=torch.int32, device=dev),
               "valid_count": torch.empty(B, dtype=torch.int32, device=dev), "status": torch.empty(B, dtype=torch.int32, device=dev)}
        ws_bytes = lib.ws3d_scan_prepare_workspace_bytes(B, up["total"])
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
        s6 = _scope6(area_scope)
        rc = lib.ws3d_scan_prepare(B, up["offsets"].data_ptr(), up["total"], up["max_n"], up["raw"].data_ptr(), up["tables"].data_ptr(),
                                   up["hw"].data_ptr(), None if s6 is None else s6.ctypes.data, npoints, int(seed) & _M64, up["keys"].data_ptr(),
                                   key_bits, res["pts_input"].data_ptr(), res["src_index"].data_ptr(), res["valid_count"].data_ptr(),
                                   res["status"].data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
    if rc == _lib.E_UNSUPPORTED:
        return None
    _lib.check(rc, "scan_prepare")
    return res


# ----------------------------------------------------------------------------- the drivers' side
class RawScenes:
    """a ``KittiScenes`` whose items are ``raw_item``s: what the loader processes read on the device_ingest routes (files only)"""

    def __init__(self, scenes):
        self.scenes = scenes

    def __len__(self) -> int:
        return len(self.scenes)

    def __getitem__(self, index: int) -> dict:
        return self.scenes.raw_item(index)


def driver_dataset(scenes, device_ingest: str = "off"):
    """what a driver indexes for its items: the scenes themselves (sampled on the host as ever) or their raw items"""
    if device_ingest not in ROUTES:
        raise ValueError(f"device_ingest must be one of {ROUTES}, got {device_ingest!r}")
    return scenes if device_ingest == "off" else RawScenes(scenes)


def batch_points(items: Sequence[dict], device_ingest: str, npoints: int, seed: int, device):
    """the (B, npoints, 4) float32 batch of a driver's items: 'off' -> the host array of the items' own ``pts_input`` (as before);
    'device' / 'host' -> a tensor on `device` prepared from the raw items with scene_key = sample id, by the kernel or by the host
    restatement (the same rows)"""
    if device_ingest == "off":
        return kitti_io.collate_scenes(items)["pts_input"]
    import torch
    res = prepare_scans([it["pts_lidar"] for it in items], [it["calib"] for it in items], [it["img_shape"] for it in items],
                        [int(it["sample_id"]) for it in items], npoints, seed, device=device if device_ingest == "device" else "cpu")
    return res["pts_input"].to(torch.device(device))
