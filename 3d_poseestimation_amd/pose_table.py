"""Pose tables on the device: from raw joint arrays to the table the feeders read, its statistics, and the transform
between raw units and a model's space (csrc/pose_table.h has the definitions).

  prepare_poses    joint pick, camera view, root-centring                      pl_pose_prepare
                   (phase3_direct/my_HybrIK/H36_dataset.py:303-379, :209-211, :288-289)
  pose_stats       per-joint mean / std / min / max of a table, fp64            pl_pose_stats      (H36_dataset.py:214-243)
  PoseTransform    standardise / normalise and the way back                     pl_pose_affine     (:261-283, main.py:473-474)

Tables stay RAW.  A feeder given `transform_2d=` / `transform_3d=` augments the raw pose and standardises it in the launch
that builds the batch (data.py); `eval_step(..., denorm=)`, `pose_errors(..., denorm=)` and `PoseMetrics.update(..., denorm=)`
take a model's outputs back inside the launches that measure them, so MPJPE is reported in the raw units.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# the usual 17 of Human3.6M's 32 joints (H36_dataset.py:48)
H36M_17_OF_32 = (0, 1, 2, 3, 6, 7, 8, 12, 13, 14, 15, 17, 18, 19, 25, 26, 27)
MAX_SRC_JOINTS, MAX_JOINTS = 64, 32


def _table(x, name):
    """A (N, J, D) fp32 device tensor, contiguous."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    _lib.require_device_tensor(x, name)
    if x.dim() != 3 or x.shape[0] == 0 or x.shape[2] not in (2, 3):
        raise ValueError(f"{name} is (N, J, 2) or (N, J, 3), got {tuple(x.shape)}")
    return x


def prepare_poses(raw, joints=None, cameras=None, cam_ids=None, zero_centre=False, device="cuda"):
    """raw (N, Jsrc, D) -> a new (N, J, D) fp32 device table: `joints` picked (None: all), each pose moved into its camera's
    frame (D = 3: cameras (C, 7) float64 rows (tx, ty, tz, qw, qx, qy, qz) with the translation in the poses' units, cam_ids
    (N,) the camera of each row), and root-centred (zero_centre: joints 1.. minus joint 0, joint 0 zero).  One launch on
    the current stream; a raw array on the host is copied to `device` first.  A cam_id outside [0, C) gives a NaN pose."""
    raw = torch.as_tensor(raw)
    if not raw.is_cuda:
        raw = raw.to(device=device, dtype=torch.float32)
    raw = _table(raw.float().contiguous(), "raw")
    N, jsrc, D = raw.shape
    pick = None
    J = jsrc
    if joints is not None:
        joints = [int(j) for j in joints]
        J = len(joints)
        pick = (ctypes.c_int32 * J)(*joints)
    if (cameras is None) != (cam_ids is None):
        raise ValueError("cameras and cam_ids come together")
    cam_t = ids_t = None
    C = 0
    if cameras is not None:
        cam_t = torch.as_tensor(cameras, dtype=torch.float64).to(raw.device).contiguous()
        if cam_t.dim() != 2 or cam_t.shape[1] != 7 or cam_t.shape[0] == 0:
            raise ValueError(f"cameras is (C, 7): translation and quaternion (w, x, y, z), got {tuple(cam_t.shape)}")
        ids_t = torch.as_tensor(cam_ids).to(device=raw.device, dtype=torch.int32).contiguous()
        if ids_t.shape != (N,):
            raise ValueError("cam_ids holds one camera index per pose")
        C = cam_t.shape[0]
    out = torch.empty((N, J, D), dtype=torch.float32, device=raw.device)
    with _lib.on_device(raw.device):
        rc = _lib.lib().pl_pose_prepare(raw.data_ptr(), N, jsrc, D, pick, J, ids_t.data_ptr() if ids_t is not None else None,
                                        cam_t.data_ptr() if cam_t is not None else None, C, int(bool(zero_centre)),
                                        out.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_pose_prepare")
    return out


class PoseStats:
    """mean, std, min, max of a pose table per joint and coordinate: four (J, D) float64 tensors on the host."""

    def __init__(self, mean, std, min, max):  # noqa: A002  (the reference's names)
        vals = [torch.as_tensor(np.asarray(v, dtype=np.float64) if not isinstance(v, torch.Tensor) else v).double().cpu()
                for v in (mean, std, min, max)]
        if vals[0].dim() != 2 or any(v.shape != vals[0].shape for v in vals):
            raise ValueError("PoseStats: mean, std, min and max are four (J, D) arrays of one shape")
        self.mean, self.std, self.min, self.max = vals

    @property
    def dim(self):
        return self.mean.shape[1]

    def _keys(self):
        d = self.dim
        return {f"mean_train_{d}d": self.mean, f"std_train_{d}d": self.std, f"min_train_{d}d": self.min,
                f"max_train_{d}d": self.max}

    def save(self, path):
        """An .npz whose keys are the reference's file names (H36_dataset.py:225-243: mean_train_3d, std_train_3d, ...)."""
        with open(path, "wb") as f:
            np.savez(f, **{k: v.numpy() for k, v in self._keys().items()})

    @classmethod
    def load(cls, path, dim=None):
        """What save() wrote; dim picks the 2-D or the 3-D record of a file that holds both (None: the only one)."""
        with np.load(path) as z:
            dims = [d for d in (2, 3) if f"mean_train_{d}d" in z.files]
            if dim is None:
                if len(dims) != 1:
                    raise ValueError(f"{path} holds statistics for D in {dims}: say which with dim=")
                dim = dims[0]
            return cls(*(z[f"{k}_train_{dim}d"] for k in ("mean", "std", "min", "max")))

    @classmethod
    def from_npz(cls, path, dim):
        """mean_train_{dim}d / std_train_{dim}d of a file that has no min / max (those become NaN)."""
        with np.load(path) as z:
            mean, std = z[f"mean_train_{dim}d"], z[f"std_train_{dim}d"]
            nan = np.full(mean.shape, np.nan)
            mn = z[f"min_train_{dim}d"] if f"min_train_{dim}d" in z.files else nan
            mx = z[f"max_train_{dim}d"] if f"max_train_{dim}d" in z.files else nan
            return cls(mean, std, mn, mx)


def pose_stats_record(table):
    """The [4][J D] fp64 device record (mean, std, min, max) of a (N, J, D) table: four launches, no host read."""
    table = _table(table, "table")
    N, W = table.shape[0], table.shape[1] * table.shape[2]
    L = _lib.lib()
    out = torch.empty((4, W), dtype=torch.float64, device=table.device)
    scratch = torch.empty(max(8, L.pl_pose_stats_scratch_bytes(N, W)) // 8, dtype=torch.float64, device=table.device)
    with _lib.on_device(table.device):
        rc = L.pl_pose_stats(table.data_ptr(), N, W, out.data_ptr(), scratch.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_pose_stats")
    return out


def pose_stats(table):
    """PoseStats of a (N, J, D) device table, J D <= 96: fp64 sums in a fixed order (the same table gives the same bits),
    the population std about the mean (H36_dataset.py:215-222); one host read."""
    rec = pose_stats_record(table).cpu().reshape((4,) + tuple(table.shape[1:]))
    return PoseStats(rec[0], rec[1], rec[2], rec[3])


class PoseTransform:
    """y = (x - sub) / div per joint and coordinate, and back: sub, div (J, D), kept as fp32.  A column with div == 0
    applies to 0 and inverts to sub (the zeroed root joint, any constant column)."""

    def __init__(self, sub, div):
        sub = torch.as_tensor(np.asarray(sub) if not isinstance(sub, torch.Tensor) else sub).detach().cpu()
        div = torch.as_tensor(np.asarray(div) if not isinstance(div, torch.Tensor) else div).detach().cpu()
        if sub.dim() != 2 or sub.shape != div.shape or sub.shape[1] not in (2, 3) or not 1 <= sub.shape[0] <= MAX_JOINTS:
            raise ValueError(f"PoseTransform: sub and div are (J, 2) or (J, 3), J <= {MAX_JOINTS}, got {tuple(sub.shape)} "
                             f"and {tuple(div.shape)}")
        self.sub, self.div = sub.to(torch.float32).contiguous(), div.to(torch.float32).contiguous()
        if not (torch.isfinite(self.sub).all() and torch.isfinite(self.div).all()):
            raise ValueError("PoseTransform: sub and div must be finite (in fp32)")
        self._dev = {}

    @classmethod
    def standardize(cls, stats):
        """(x - mean) / std of a PoseStats (H36_dataset.py:272, :283)."""
        return cls(stats.mean, stats.std)

    @classmethod
    def normalize_2d(cls, joints=17):
        """2 x - 1 (H36_dataset.py:269), as (x - 0.5) / 0.5: the same bits for x in [0, 1]."""
        return cls(torch.full((joints, 2), 0.5), torch.full((joints, 2), 0.5))

    @classmethod
    def normalize_3d(cls, lo=-1.0, hi=1.0, joints=17):
        """(x - lo) / (hi - lo) - 0.5 (H36_dataset.py:279-280), as (x - (lo + hi) / 2) / (hi - lo)."""
        lo = torch.as_tensor(lo, dtype=torch.float64).expand(joints, 3)
        hi = torch.as_tensor(hi, dtype=torch.float64).expand(joints, 3)
        return cls((lo + hi) / 2, hi - lo)

    @property
    def shape(self):
        return tuple(self.sub.shape)

    def device_pair(self, device):
        """(sub, div) on `device`, copied there once."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        pair = self._dev.get(device)
        if pair is None:
            pair = self._dev[device] = (self.sub.to(device), self.div.to(device))
        return pair

    def _run(self, x, invert, out):
        if not isinstance(x, torch.Tensor):
            raise TypeError("PoseTransform works on device tensors")
        _lib.require_device_tensor(x, "x")
        if x.dim() < 2 or tuple(x.shape[-2:]) != self.shape:
            raise ValueError(f"PoseTransform of shape {self.shape} cannot take a tensor of shape {tuple(x.shape)}")
        if x.numel() == 0:
            raise ValueError("PoseTransform: empty tensor")
        W = self.shape[0] * self.shape[1]
        sub, div = self.device_pair(x.device)
        y = x if out is None else out
        with _lib.on_device(x.device):
            rc = _lib.lib().pl_pose_affine(x.data_ptr(), x.numel() // W, W, sub.data_ptr(), div.data_ptr(), int(invert),
                                           y.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_pose_affine")
        return y

    def apply(self, x):
        """(x - sub) / div as a new tensor; x (..., J, D) on the device."""
        return self._run(x, False, torch.empty_like(x))

    def invert(self, y):
        """y div + sub as a new tensor."""
        return self._run(y, True, torch.empty_like(y))

    def apply_(self, x):
        return self._run(x, False, None)

    def invert_(self, y):
        return self._run(y, True, None)


def transform_pair(transform, shape, device, what):
    """(sub, div) device pointers of an optional PoseTransform for poses of `shape` (J, D); (None, None) without one.
    The tensors are returned too, so the caller keeps them alive across the launch."""
    if transform is None:
        return None, None, None
    if not isinstance(transform, PoseTransform):
        raise TypeError(f"{what} must be a PoseTransform or None")
    if transform.shape != tuple(shape):
        raise ValueError(f"{what} has shape {transform.shape}, the poses {tuple(shape)}")
    pair = transform.device_pair(device)
    return pair[0].data_ptr(), pair[1].data_ptr(), pair
