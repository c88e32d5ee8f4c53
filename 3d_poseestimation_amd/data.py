"""Batch feeder for the lifter step: replaces the reference's DataLoader hop
(/root/reference/phase1_lifting/train_1.py:26-31 `DataLoader(training_set, shuffle=True, batch_size=...)`,
:75-81 `.float()`, `.to(device)`) for pose tables that are already arrays.

The MI355X answer to "load a batch" is not to load it: Human3.6M's ~1.5 M training poses are
(17*2 + 17*3) * 4 B = 340 B each, 0.5 GB -- 0.2 % of the 288 GB of HBM.  `PoseFeeder` keeps both
tables resident and a batch is a device-side row gather by the epoch's permutation
(pl_gather_rows2): no per-step H2D copy, no host synchronisation, nothing for the train step to
wait on.  Tables that should not be resident (`resident=False`) stay in pinned host memory and
batches are gathered on the host into pinned staging buffers and copied on a side stream two
batches ahead; the consumer only waits on an event.

Data parallel: every rank draws the same permutation (same seed) and takes its `dp.shard_rows`
slice of each global batch of `batch_size * world` rows.

Train-time augmentation (`PoseAugment`: horizontal flip, in-plane rotation, 2-D scale, shift and Gaussian jitter; the
reference's commented-out H36_dataset.py:98-117 and train_1.py:83-84) happens inside the launch that builds the batch
(pl_pose_augment_gather, csrc/pose_augment.h).  Every draw of a pose is a function of (seed, epoch, dataset row), so a run
replays bit for bit under another batch size, rank count or feeder mode.

Tables stay raw.  `transform_2d=` / `transform_3d=` (pose_table.PoseTransform: standardise, normalise) are applied to each
batch AFTER the augmentation, in the same launch (pl_pose_augment_gather_t): a flip of standardised coordinates is no
mirror image unless the statistics are left/right symmetric, and jitter, shift and centre are in image units.

Frames (`FrameFeeder`, `augment_frames`): the image networks read [B,256,256,3] fp32 NHWC frames that the reference prepares per
sample on DataLoader workers (H36_dataset.py:129-131 `cv2.resize(frame,(256,256))`, `frame/256.0`).  Here the frames stay a
uint8 table -- a quarter of the fp32 bytes, resident or pinned -- and one launch (pl_frame_warp_gather, csrc/frame_warp.h)
gathers, resizes, scales and warps a batch by the very draws its poses get: frame, 2-D pose and 3-D pose of a dataset row
always agree.

Person-centred crops (`PersonCrop`, `crop=`): the reference's "cropping using the gt 2d as bounding box" (H36_dataset.py:120-126)
always selects the whole frame.  With a crop both launches take a square box from the row's source 2-D pose (csrc/frame_crop.h,
the same inline text in both, so they agree bit for bit): the frame launch resizes the box instead of the frame, the pose
launch puts the 2-D pose into crop coordinates in front of the augmentation and writes the boxes, which `uncrop_poses` /
`crop_poses` (train.py) use to move predictions between crop and image coordinates.
"""
import ctypes
import dataclasses
import math

import torch

from . import _lib
from .dp import shard_rows
from .pose_table import transform_pair


def epoch_indices(n_rows, batch_size, *, epoch=0, seed=0, shuffle=True, drop_last=False, rank=0, world=1):
    """The index tensors (int64, CPU) of this rank's batches for one epoch.  A global batch is
    `batch_size * world` consecutive entries of the epoch's permutation; the last one may be short
    (DataLoader's drop_last=False).  With world > 1 every rank must run the same number of steps on the
    same number of rows (the gradient all-reduce and SyncBN are collectives; training-mode BatchNorm needs
    >= 2 rows): the short tail batch is trimmed to a multiple of `world` rows and dropped on EVERY rank when
    that leaves fewer than 2 rows per rank."""
    if n_rows <= 0 or batch_size <= 0 or not (0 <= rank < world):
        raise ValueError("bad feeder geometry")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) * 1000003 + int(epoch))
        perm = torch.randperm(n_rows, generator=g)
    else:
        perm = torch.arange(n_rows)
    gb = batch_size * world
    out = []
    for start in range(0, n_rows, gb):
        chunk = perm[start:start + gb]
        if chunk.numel() < gb and drop_last:
            break
        if world > 1 and chunk.numel() < gb:
            per = chunk.numel() // world
            if per < 2:
                break
            chunk = chunk[:per * world]
        lo, hi = shard_rows(chunk.numel(), rank, world)
        out.append(chunk[lo:hi])
    return out


def epoch_steps(n_rows, batch_size, *, drop_last=False, world=1):
    """Number of batches epoch_indices() yields -- the same on every rank."""
    gb = batch_size * world
    full, tail = divmod(n_rows, gb)
    if drop_last or tail == 0:
        return full
    return full + (1 if (world == 1 or tail // world >= 2) else 0)


@dataclasses.dataclass(frozen=True)
class PoseAugment:
    """Seeded train-time augmentation of (17,2)/(17,3) pose pairs (csrc/pose_augment.h has the definition).

    2-D: flip (flip_pose's joint swap, x -> flip_offset - x) with probability p_flip, rotate about `centre` by an angle
    uniform in [-max_rot, max_rot) radians, scale about `centre` by a factor uniform in [1 - scale_range, 1 + scale_range),
    shift by (tx, ty) uniform in [-max_shift, max_shift), add N(0, jitter_sigma^2) noise to every coordinate.
    3-D: the same flip (x -> -x) and the same rotation of (x, y); z, scale and shift leave the root-relative target alone.
    flip_offset is 1 for image-normalised x in [0, 1].  Augment RAW poses: keep the tables raw and pass the feeder (or
    augment_poses) `transform_2d=` / `transform_3d=`, which standardise the batch after the augmentation in the same
    launch -- on standardised coordinates the flip is no mirror image and the other parameters lose their units.  A
    parameter of 0 switches its stage off exactly; the default object changes no bit."""
    p_flip: float = 0.0
    flip_offset: float = 1.0
    max_rot: float = 0.0
    scale_range: float = 0.0
    max_shift: float = 0.0
    jitter_sigma: float = 0.0
    centre: tuple = (0.5, 0.5)
    seed: int = 0

    def __post_init__(self):
        centre = tuple(float(c) for c in self.centre)
        if len(centre) != 2:
            raise ValueError("centre is (cx, cy)")
        object.__setattr__(self, "centre", centre)
        for name in ("p_flip", "flip_offset", "max_rot", "scale_range", "max_shift", "jitter_sigma"):
            object.__setattr__(self, name, float(getattr(self, name)))
        for name, v in (("flip_offset", self.flip_offset), ("cx", centre[0]), ("cy", centre[1])):
            if not math.isfinite(v):
                raise ValueError(f"{name} must be finite")
        for name in ("p_flip", "max_rot", "scale_range", "max_shift", "jitter_sigma"):
            v = getattr(self, name)
            if not math.isfinite(v) or v < 0.0:
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        if self.scale_range >= 1.0:
            raise ValueError("scale_range must be below 1")
        seed = int(self.seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed is a uint64")
        object.__setattr__(self, "seed", seed)

    def struct(self):
        """The PLPoseAug the library reads."""
        return _lib.PLPoseAug(self.p_flip, self.flip_offset, self.max_rot, self.scale_range, self.max_shift,
                              self.jitter_sigma, self.centre[0], self.centre[1], self.seed)


@dataclasses.dataclass(frozen=True)
class PersonCrop:
    """Person-centred square crop taken from each row's 2-D pose (csrc/frame_crop.h has the definition).

    The box of a row comes from its SOURCE image-normalised 2-D pose and the source frame size: its side is `margin` times
    the larger extent of the 17 joints in source pixels, rounded up, at least `min_side`; it is centred on the middle of the
    extent (centre="bbox") or on joint 0 (centre="root", what the reference's dead crop aimed at), and its corner is rounded
    to whole source pixels.  The part of a box outside the frame is `fill`.  The 2-D pose goes into crop coordinates
    ([0, 1] across the box) in front of every augmentation stage, so a PoseAugment's centre (0.5, 0.5) is the crop's centre;
    the 3-D pose is untouched.  A pose with a non-finite coordinate, or a side above 2^20, gives a NaN box, frame and 2-D pose."""
    margin: float = 1.25
    centre: str = "bbox"
    min_side: int = 8

    def __post_init__(self):
        margin = float(self.margin)
        if not math.isfinite(margin) or margin <= 0.0:
            raise ValueError(f"margin must be finite and > 0, got {margin}")
        object.__setattr__(self, "margin", margin)
        if self.centre not in ("bbox", "root"):
            raise ValueError(f"centre is 'bbox' or 'root', got {self.centre!r}")
        if float(self.min_side) != int(self.min_side) or not 1 <= int(self.min_side) <= 2 ** 20:
            raise ValueError(f"min_side is an integer in [1, 2^20], got {self.min_side}")
        object.__setattr__(self, "min_side", int(self.min_side))

    def struct(self, frame_hw):
        """The PLPoseCrop the library reads, for source frames of frame_hw = (Hs, Ws)."""
        hs, ws = (int(v) for v in frame_hw)
        if hs <= 0 or ws <= 0:
            raise ValueError("frame_hw is (Hs, Ws), both positive")
        return _lib.PLPoseCrop(self.margin, _lib.CROP_ROOT if self.centre == "root" else _lib.CROP_BBOX, float(self.min_side),
                               0, hs, ws)


def _crop_struct(crop, frame_hw, augment=None):
    """The PLPoseCrop of a PersonCrop (None: no crop), with the check a flip needs."""
    if crop is None:
        return None
    if not isinstance(crop, PersonCrop):
        raise TypeError("crop must be a PersonCrop or None")
    if frame_hw is None:
        raise ValueError("a crop needs frame_hw = (Hs, Ws), the source frames' size")
    if augment is not None and augment.p_flip > 0.0 and augment.flip_offset != 1.0:
        raise ValueError("a flip of a cropped pose mirrors about the crop's centre: p_flip > 0 needs flip_offset = 1, got "
                         f"{augment.flip_offset}")
    return crop.struct(frame_hw)


def _augment_launch(a, b, src_idx, row_ids, nb, table_rows, oa, ob, aug_struct, epoch, xf=None, crop=None, boxes=None):
    """One pl_pose_augment_gather on torch's current stream; src_idx None = the rows of a, b in order.
    xf: (sub_a, div_a, sub_b, div_b) device pointers of the transforms (_transforms) -> pl_pose_augment_gather_t.
    crop: a PLPoseCrop and boxes its (nb, 4) output -> the _crop forms of the same two entry points."""
    if crop is not None:
        L, src = _lib.lib(), src_idx.data_ptr() if src_idx is not None else None
        if xf is not None:
            _lib.check(L.pl_pose_augment_gather_crop_t(a.data_ptr(), b.data_ptr(), src, row_ids.data_ptr(), nb, table_rows,
                                                       oa.data_ptr(), ob.data_ptr(), ctypes.byref(aug_struct), int(epoch),
                                                       xf[0], xf[1], xf[2], xf[3], ctypes.byref(crop), boxes.data_ptr(),
                                                       _lib.current_stream_ptr()), "pl_pose_augment_gather_crop_t")
        else:
            _lib.check(L.pl_pose_augment_gather_crop(a.data_ptr(), b.data_ptr(), src, row_ids.data_ptr(), nb, table_rows,
                                                     oa.data_ptr(), ob.data_ptr(), ctypes.byref(aug_struct), int(epoch),
                                                     ctypes.byref(crop), boxes.data_ptr(), _lib.current_stream_ptr()),
                       "pl_pose_augment_gather_crop")
        return
    if xf is not None:
        _lib.check(_lib.lib().pl_pose_augment_gather_t(a.data_ptr(), b.data_ptr(),
                                                       src_idx.data_ptr() if src_idx is not None else None,
                                                       row_ids.data_ptr(), nb, table_rows, oa.data_ptr(), ob.data_ptr(),
                                                       ctypes.byref(aug_struct), int(epoch), xf[0], xf[1], xf[2], xf[3],
                                                       _lib.current_stream_ptr()),
                   "pl_pose_augment_gather_t")
        return
    _lib.check(_lib.lib().pl_pose_augment_gather(a.data_ptr(), b.data_ptr(), src_idx.data_ptr() if src_idx is not None else None,
                                                 row_ids.data_ptr(), nb, table_rows, oa.data_ptr(), ob.data_ptr(),
                                                 ctypes.byref(aug_struct), int(epoch), _lib.current_stream_ptr()),
               "pl_pose_augment_gather")


def _transforms(transform_2d, transform_3d, device):
    """((sub_a, div_a, sub_b, div_b), tensors kept alive) of the optional pair; (None, None) when both are None."""
    if transform_2d is None and transform_3d is None:
        return None, None
    sa, da, keep_a = transform_pair(transform_2d, (17, 2), device, "transform_2d")
    sb, db, keep_b = transform_pair(transform_3d, (17, 3), device, "transform_3d")
    return (sa, da, sb, db), (keep_a, keep_b)


def augment_poses(y1, y2, augment, row_ids=None, epoch=0, transform_2d=None, transform_3d=None, crop=None, frame_hw=None):
    """`augment` applied to a batch that came from somewhere else: y1 (B,17,2), y2 (B,17,3) fp32 device tensors -> new
    (y1, y2) tensors; the inputs are untouched and nothing synchronises (one launch on the current stream).

    A pose's draws are a function of (augment.seed, epoch, row id) only.  Pass the poses' DATASET indices as `row_ids`
    (int64, B of them) -- or at least an `epoch` that changes from call to call -- to get fresh draws: with the default
    row_ids = arange(B) and a fixed epoch, pose k of every batch is flipped, turned and jittered the same way.
    transform_2d / transform_3d: PoseTransforms applied to the augmented poses in the same launch.
    crop: a PersonCrop, with frame_hw = (Hs, Ws) of the source frames: y1 goes into the crop coordinates of its own box in
    front of the augmentation (a transform_2d then needs statistics of crop coordinates) and the call returns
    (y1, y2, boxes), boxes (B,4) fp32 = (x0, y0, side, side) in source pixels -- what uncrop_poses takes."""
    if not isinstance(augment, PoseAugment):
        raise TypeError("augment must be a PoseAugment")
    crop_s = _crop_struct(crop, frame_hw, augment)
    _lib.require_device_tensor(y1, "y1")
    _lib.require_device_tensor(y2, "y2")
    if y1.dim() != 3 or y2.dim() != 3 or tuple(y1.shape[1:]) != (17, 2) or tuple(y2.shape[1:]) != (17, 3) \
            or y1.shape[0] != y2.shape[0] or y1.shape[0] == 0 or y1.device != y2.device:
        raise ValueError("augment_poses expects y1 (B,17,2) and y2 (B,17,3) on one device, B >= 1")
    nb = y1.shape[0]
    if row_ids is None:
        row_ids = torch.arange(nb, dtype=torch.int64, device=y1.device)
    else:
        row_ids = torch.as_tensor(row_ids).to(device=y1.device, dtype=torch.int64).contiguous()
        if row_ids.shape != (nb,):
            raise ValueError("row_ids holds one dataset index per pose")
    oa, ob = torch.empty_like(y1), torch.empty_like(y2)
    xf, _keep = _transforms(transform_2d, transform_3d, y1.device)
    boxes = torch.empty((nb, 4), dtype=torch.float32, device=y1.device) if crop_s is not None else None
    with _lib.on_device(y1.device):
        _augment_launch(y1, y2, None, row_ids, nb, nb, oa, ob, augment.struct(), epoch, xf, crop_s, boxes)
    return (oa, ob) if boxes is None else (oa, ob, boxes)


def _weights_launch(w, src_idx, row_ids, nb, table_rows, J, out, aug_struct, epoch):
    """One pl_row_weights_gather on torch's current stream; src_idx None = the rows of w in order, aug_struct None = no flip"""
    _lib.check(_lib.lib().pl_row_weights_gather(w.data_ptr(), src_idx.data_ptr() if src_idx is not None else None,
                                                row_ids.data_ptr() if row_ids is not None else None, nb, table_rows, J,
                                                out.data_ptr(), ctypes.byref(aug_struct) if aug_struct is not None else None,
                                                int(epoch), _lib.current_stream_ptr()), "pl_row_weights_gather")


def gather_row_weights(table_or_batch, augment=None, row_ids=None, epoch=0, src_idx=None):
    """The per-pose joint weights (PoseCriterion's row_weights) of a batch that augment_poses built: the companion call for
    batches from another loader.  table_or_batch (N, J) device tensor -> (B, J) fp32, out[k] = table[src_idx[k]] (src_idx
    None: the rows in order, B = N) with the left / right joints swapped where `augment` (the PoseAugment given to
    augment_poses, with the same row_ids and epoch) flipped pose k -- the weights follow the joints; no other stage moves
    a joint.  augment None or p_flip = 0: a plain gather, any J; otherwise J = 17.  One small launch, nothing synchronises;
    a src_idx outside the table gives a NaN row."""
    if augment is not None and not isinstance(augment, PoseAugment):
        raise TypeError("augment must be a PoseAugment or None")
    _lib.require_device_tensor(table_or_batch, "table_or_batch")
    if table_or_batch.dim() != 2 or table_or_batch.shape[0] == 0 or table_or_batch.shape[1] == 0:
        raise ValueError("gather_row_weights expects a (N, J) table, N, J >= 1")
    w = table_or_batch.float().contiguous()
    n, J = w.shape
    if augment is not None and augment.p_flip > 0.0 and J != 17:
        raise ValueError(f"a flip swaps the left and right of 17 joints, the table has {J}")
    if src_idx is not None:
        src_idx = torch.as_tensor(src_idx).to(device=w.device, dtype=torch.int64).contiguous()
        if src_idx.dim() != 1 or src_idx.numel() == 0:
            raise ValueError("src_idx holds one table row per pose")
    nb = src_idx.numel() if src_idx is not None else n
    if row_ids is None:
        row_ids = src_idx if src_idx is not None else torch.arange(nb, dtype=torch.int64, device=w.device)
    else:
        row_ids = torch.as_tensor(row_ids).to(device=w.device, dtype=torch.int64).contiguous()
        if row_ids.shape != (nb,):
            raise ValueError("row_ids holds one dataset index per pose")
    out = torch.empty((nb, J), dtype=torch.float32, device=w.device)
    with _lib.on_device(w.device):
        _weights_launch(w, src_idx, row_ids, nb, n, J, out, augment.struct() if augment is not None else None, epoch)
    return out


def crop_boxes(x2d, crop, frame_hw):
    """The boxes (B,4) fp32 = (x0, y0, side, side), in source pixels, that `crop` (a PersonCrop) takes from the
    image-normalised 2-D poses x2d (B,17,2) of frames of frame_hw = (Hs, Ws): the boxes the feeder's two launches compute for
    the same rows, bit for bit.  One launch on the current stream."""
    crop_s = _crop_struct(crop, frame_hw)
    if crop_s is None:
        raise TypeError("crop must be a PersonCrop")
    _lib.require_device_tensor(x2d, "x2d")
    if x2d.dim() != 3 or tuple(x2d.shape[1:]) != (17, 2) or x2d.shape[0] == 0:
        raise ValueError("crop_boxes expects x2d (B,17,2), B >= 1")
    boxes = torch.empty((x2d.shape[0], 4), dtype=torch.float32, device=x2d.device)
    with _lib.on_device(x2d.device):
        _lib.check(_lib.lib().pl_pose_crop_boxes(x2d.data_ptr(), x2d.shape[0], ctypes.byref(crop_s), boxes.data_ptr(),
                                                 _lib.current_stream_ptr()), "pl_pose_crop_boxes")
    return boxes


class PoseFeeder:
    """Iterable of (y1 [b,17,2], y2 [b,17,3]) fp32 device batches over one epoch; call
    set_epoch(e) between epochs (as with DistributedSampler) for a fresh permutation.
    augment: a PoseAugment applied inside the launch that builds the batch, with the epoch of set_epoch and the poses'
    dataset rows as the identity of the draws (None: the plain gather).
    transform_2d / transform_3d: PoseTransforms (pose_table) applied to every batch after the augmentation, in the same
    launch; the tables stay raw.  With a transform and no augmentation the batch is built by the augmented gather with
    every stage off: a copy plus the transform, still one launch.
    crop: a PersonCrop with frame_hw = (Hs, Ws) of the source frames: the batches are (y1, y2, boxes), y1 in the crop
    coordinates of its own box (in front of the augmentation, same launch) and boxes (b,4) fp32 on the device.
    weights: a (N, J) table of per-pose joint weights (visibility, confidence; PoseCriterion's row_weights), resident or
    pinned like the pose tables (streamed: it rides the same staged copy).  Every batch tuple gains w (b, J) fp32 as its
    LAST item -- after boxes when there is a crop -- built by one small launch more (pl_row_weights_gather) from the batch's
    rows and the epoch of set_epoch: where the augmentation flipped a pose its weights swap left and right with the joints
    (J = 17 with a flip); without an augmentation it is the plain table[idx]."""

    def __init__(self, x2d, y3d, batch_size, *, device="cuda", shuffle=True, seed=0, drop_last=False,
                 rank=0, world=1, resident=True, prefetch=2, augment=None, transform_2d=None, transform_3d=None,
                 crop=None, frame_hw=None, weights=None):
        x2d, y3d = torch.as_tensor(x2d), torch.as_tensor(y3d)
        if x2d.shape[0] != y3d.shape[0] or x2d.shape[0] == 0:
            raise ValueError("x2d and y3d need the same, non-zero number of poses")
        self.n = x2d.shape[0]
        self.shape_a, self.shape_b = tuple(x2d.shape[1:]), tuple(y3d.shape[1:])
        if augment is not None:
            if not isinstance(augment, PoseAugment):
                raise TypeError("augment must be a PoseAugment or None")
            if self.shape_a != (17, 2) or self.shape_b != (17, 3):
                raise ValueError(f"augmentation is defined for (N,17,2)/(N,17,3) tables, got {tuple(x2d.shape)} / "
                                 f"{tuple(y3d.shape)}")
        self.augment = augment
        self._aug = augment.struct() if augment is not None else None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PoseliftError("PoseFeeder feeds an MI355X (ROCm) device; there is no CPU path")
        self.transform_2d, self.transform_3d = transform_2d, transform_3d
        self._xf = self._xf_keep = None
        if transform_2d is not None or transform_3d is not None:
            if self.shape_a != (17, 2) or self.shape_b != (17, 3):
                raise ValueError(f"transforms ride in the augmented gather, defined for (N,17,2)/(N,17,3) tables, got "
                                 f"{tuple(x2d.shape)} / {tuple(y3d.shape)}")
            self._xf, self._xf_keep = _transforms(transform_2d, transform_3d, self.device)
            if self._aug is None:
                self._aug = PoseAugment().struct()          # every stage off: the kernel copies, then transforms
        self.crop = crop
        self._crop = _crop_struct(crop, frame_hw, augment)
        if self._crop is not None:
            if self.shape_a != (17, 2) or self.shape_b != (17, 3):
                raise ValueError(f"a crop rides in the augmented gather, defined for (N,17,2)/(N,17,3) tables, got "
                                 f"{tuple(x2d.shape)} / {tuple(y3d.shape)}")
            if self._aug is None:
                self._aug = PoseAugment().struct()          # every stage off: the kernel crops and copies
        a = x2d.reshape(self.n, -1).to(torch.float32).contiguous()        # train_1.py:80 .float()
        b = y3d.reshape(self.n, -1).to(torch.float32).contiguous()
        self.wa, self.wb = a.shape[1], b.shape[1]
        self.batch_size, self.shuffle, self.seed, self.drop_last = batch_size, shuffle, seed, drop_last
        self.rank, self.world, self.resident, self.prefetch = rank, world, resident, max(1, int(prefetch))
        self.epoch = 0
        self.w = None
        if weights is not None:
            w = torch.as_tensor(weights)
            if w.dim() != 2 or w.shape[0] != self.n or w.shape[1] < 1:
                raise ValueError(f"weights is a (N, J) table with one row per pose, got {tuple(w.shape)} for {self.n} poses")
            if augment is not None and augment.p_flip > 0.0 and w.shape[1] != 17:
                raise ValueError(f"a flip swaps the left and right of 17 joints, the weights table has {w.shape[1]}")
            self.w = w.to(torch.float32).contiguous()
            self.wj = self.w.shape[1]
        # (the weights see the flip of the batch's augmentation and nothing else of it; no augmentation: no flip)
        self._waug = augment.struct() if augment is not None else None
        if resident:
            self.a, self.b = a.to(self.device), b.to(self.device)
            self.w = self.w.to(self.device) if self.w is not None else None
        else:
            self.a, self.b = a.pin_memory(), b.pin_memory()
            self.w = self.w.pin_memory() if self.w is not None else None
            self._copy_stream = torch.cuda.Stream(self.device)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _indices(self):
        return epoch_indices(self.n, self.batch_size, epoch=self.epoch, seed=self.seed, shuffle=self.shuffle,
                             drop_last=self.drop_last, rank=self.rank, world=self.world)

    def __len__(self):
        return epoch_steps(self.n, self.batch_size, drop_last=self.drop_last, world=self.world)

    def __iter__(self):
        return self._iter_resident() if self.resident else self._iter_streamed()

    def _iter_resident(self):
        batches, epoch = self._indices(), self.epoch
        if not batches:
            return
        # one H2D of the whole epoch's permutation (8 B per pose), then only device work
        sizes = [t.numel() for t in batches]
        idx_all = torch.cat(batches).to(self.device, non_blocking=True)
        L, at = _lib.lib(), 0
        for nb in sizes:
            oa = torch.empty((nb,) + self.shape_a, dtype=torch.float32, device=self.device)
            ob = torch.empty((nb,) + self.shape_b, dtype=torch.float32, device=self.device)
            with _lib.on_device(self.device):
                if self._aug is not None:           # the permutation slice is both the source row and the draws' identity
                    idx = idx_all[at:at + nb]
                    boxes = torch.empty((nb, 4), dtype=torch.float32, device=self.device) if self._crop is not None else None
                    _augment_launch(self.a, self.b, idx, idx, nb, self.n, oa, ob, self._aug, epoch, self._xf, self._crop, boxes)
                else:
                    _lib.check(L.pl_gather_rows2(self.a.data_ptr(), self.wa, self.b.data_ptr(), self.wb,
                                                 idx_all[at:at + nb].data_ptr(), nb, self.n, oa.data_ptr(), ob.data_ptr(),
                                                 _lib.current_stream_ptr()), "pl_gather_rows2")
                if self.w is not None:
                    idx = idx_all[at:at + nb]
                    ow = torch.empty((nb, self.wj), dtype=torch.float32, device=self.device)
                    _weights_launch(self.w, idx, idx, nb, self.n, self.wj, ow, self._waug, epoch)
            at += nb
            out = (oa, ob, boxes) if self._crop is not None else (oa, ob)
            yield out + (ow,) if self.w is not None else out

    def _iter_streamed(self):
        batches, epoch = self._indices(), self.epoch
        slots, inflight = self.prefetch + 1, []
        stage = [(torch.empty(self.batch_size, self.wa).pin_memory(), torch.empty(self.batch_size, self.wb).pin_memory())
                 for _ in range(slots)]
        free_events = [None] * slots                      # consumer done with the slot's previous batch
        # augmentation: the batch's dataset rows ride the same copy (8 B per pose); they are the identity of its draws
        stage_idx = [torch.empty(self.batch_size, dtype=torch.int64).pin_memory() for _ in range(slots)] \
            if self._aug is not None else None
        stage_w = [torch.empty(self.batch_size, self.wj).pin_memory() for _ in range(slots)] if self.w is not None else None

        def launch(k, idx):
            slot = k % slots
            nb = idx.numel()
            ha, hb = stage[slot][0][:nb], stage[slot][1][:nb]
            if free_events[slot] is not None:
                free_events[slot].synchronize()           # staging buffer no longer being copied from
            torch.index_select(self.a, 0, idx, out=ha)
            torch.index_select(self.b, 0, idx, out=hb)
            hw = None
            if stage_w is not None:
                hw = stage_w[slot][:nb]
                torch.index_select(self.w, 0, idx, out=hw)
            with torch.cuda.stream(self._copy_stream):
                da = ha.to(self.device, non_blocking=True).view((nb,) + self.shape_a)
                db = hb.to(self.device, non_blocking=True).view((nb,) + self.shape_b)
                dw = hw.to(self.device, non_blocking=True) if hw is not None else None
                di = None
                if stage_idx is not None:
                    hi = stage_idx[slot][:nb]
                    hi.copy_(idx)
                    di = hi.to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._copy_stream)
            free_events[slot] = ev
            return da, db, di, dw, ev

        nxt = 0
        while nxt < len(batches) and len(inflight) < self.prefetch:
            inflight.append(launch(nxt, batches[nxt]))
            nxt += 1
        while inflight:
            da, db, di, dw, ev = inflight.pop(0)
            torch.cuda.current_stream(self.device).wait_event(ev)
            da.record_stream(torch.cuda.current_stream(self.device))
            db.record_stream(torch.cuda.current_stream(self.device))
            if di is not None:
                di.record_stream(torch.cuda.current_stream(self.device))
            if dw is not None:                            # (read on the consumer's stream whether or not a launch follows)
                dw.record_stream(torch.cuda.current_stream(self.device))
            if dw is not None and self._waug is not None:  # the staged rows are in batch order: only the flip is left to do
                nb = dw.shape[0]
                ow = torch.empty_like(dw)
                with _lib.on_device(self.device):
                    _weights_launch(dw, None, di, nb, nb, self.wj, ow, self._waug, epoch)
                dw = ow
            if di is not None and self._aug is not None:  # one launch on the consumer's stream, behind the event wait
                nb = di.numel()
                oa, ob = torch.empty_like(da), torch.empty_like(db)
                boxes = torch.empty((nb, 4), dtype=torch.float32, device=self.device) if self._crop is not None else None
                with _lib.on_device(self.device):
                    _augment_launch(da, db, None, di, nb, nb, oa, ob, self._aug, epoch, self._xf, self._crop, boxes)
                da, db = oa, ob
            if nxt < len(batches):
                inflight.append(launch(nxt, batches[nxt]))
                nxt += 1
            out = (da, db, boxes) if self._crop is not None else (da, db)
            yield out + (dw,) if dw is not None else out


def _frame_augment_struct(augment):
    """The PLPoseAug a frame warp reads (None: plain resize)."""
    if augment is None:
        return None
    if not isinstance(augment, PoseAugment):
        raise TypeError("augment must be a PoseAugment or None")
    if augment.p_flip > 0.0 and augment.flip_offset != 1.0:
        raise ValueError("a frame flip mirrors about the image centre: p_flip > 0 needs flip_offset = 1 "
                         f"(image-normalised 2-D poses), got {augment.flip_offset}")
    return augment.struct()


def _frame_geometry(frames, out_hw, scale, fill):
    """(dtype code, (Ho, Wo), scale, fill) of a [N,Hs,Ws,3] uint8 / fp32 frame table."""
    if frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) == 0:
        raise ValueError(f"frames are [N,Hs,Ws,3] (NHWC), got {tuple(frames.shape)}")
    if frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"frames are uint8 or float32, got {frames.dtype}")
    ho, wo = (int(v) for v in out_hw)
    if ho <= 0 or wo <= 0:
        raise ValueError("out_hw is (Ho, Wo), both positive")
    u8 = frames.dtype == torch.uint8
    if scale is None:
        scale = 1.0 / 256.0 if u8 else 1.0               # H36_dataset.py:131 frame/256.0
    return (_lib.FRAME_U8 if u8 else _lib.FRAME_F32), (ho, wo), float(scale), float(fill)


def _frame_launch(table, code, src_idx, row_ids, nb, out, scale, fill, aug_struct, epoch, crop=None, x2d=None):
    """One pl_frame_warp_gather on torch's current stream; src_idx None = the frames of `table` in order.
    crop: a PLPoseCrop and x2d the source 2-D poses, indexed like the frames -> pl_frame_warp_gather_crop."""
    args = _lib.PLFrameWarp(table.data_ptr(), code, 3, table.shape[0], table.shape[1], table.shape[2],
                            src_idx.data_ptr() if src_idx is not None else None,
                            row_ids.data_ptr() if row_ids is not None else None, nb, out.data_ptr(), out.shape[1],
                            out.shape[2], scale, fill, ctypes.pointer(aug_struct) if aug_struct is not None else None,
                            int(epoch))
    if crop is not None:
        _lib.check(_lib.lib().pl_frame_warp_gather_crop(ctypes.byref(args), ctypes.byref(crop), x2d.data_ptr(),
                                                        _lib.current_stream_ptr()), "pl_frame_warp_gather_crop")
        return
    _lib.check(_lib.lib().pl_frame_warp_gather(ctypes.byref(args), _lib.current_stream_ptr()), "pl_frame_warp_gather")


def augment_frames(frames, augment, row_ids=None, epoch=0, out_hw=(256, 256), fill=0.0, scale=None, crop=None, x2d=None):
    """`augment` applied to the frames of a batch: frames [B,Hs,Ws,3] uint8 or fp32 on the device -> a new [B,Ho,Wo,3] fp32
    tensor, resized (bilinear, cv2.resize's half-pixel convention), multiplied by `scale` (default 1/256 for uint8, the
    reference's frame/256.0, and 1 for fp32) and flipped, turned, scaled and shifted exactly as augment_poses moves the 2-D
    poses of the same (row_ids, epoch); pixels whose source lies outside the frame are `fill`.  One launch on the current
    stream, nothing synchronises.  row_ids and epoch as in augment_poses; augment=None is the plain resize.
    crop: a PersonCrop, with x2d (B,17,2) the frames' SOURCE image-normalised 2-D poses (not augment_poses' output): each
    frame is cropped to its pose's box before everything else -- the box augment_poses(crop=) and crop_boxes return."""
    aug = _frame_augment_struct(augment)
    if not isinstance(frames, torch.Tensor):
        raise TypeError("frames must be a tensor")
    code, (ho, wo), scale, fill = _frame_geometry(frames, out_hw, scale, fill)
    crop_s = _crop_struct(crop, frames.shape[1:3])
    if crop_s is not None and x2d is None:
        raise ValueError("a crop needs x2d, the frames' source 2-D poses")
    _lib.require_device_tensor(frames, "frames", dtype=frames.dtype)
    nb = frames.shape[0]
    if row_ids is None:
        row_ids = torch.arange(nb, dtype=torch.int64, device=frames.device)
    else:
        row_ids = torch.as_tensor(row_ids).to(device=frames.device, dtype=torch.int64).contiguous()
        if row_ids.shape != (nb,):
            raise ValueError("row_ids holds one dataset index per frame")
    if crop_s is not None:
        _lib.require_device_tensor(x2d, "x2d")
        if tuple(x2d.shape) != (nb, 17, 2) or x2d.device != frames.device:
            raise ValueError("x2d holds one (17,2) pose per frame, on the frames' device")
    out = torch.empty((nb, ho, wo, 3), dtype=torch.float32, device=frames.device)
    with _lib.on_device(frames.device):
        _frame_launch(frames, code, None, row_ids, nb, out, scale, fill, aug, epoch, crop_s, x2d)
    return out


class FrameFeeder:
    """Iterable of (frame [b,Ho,Wo,3], y1 [b,17,2], y2 [b,17,3]) fp32 device batches over one epoch: a PoseFeeder whose
    batches come with their frames.  frames: a [N,Hs,Ws,3] uint8 (or fp32) table, one frame per pose row.  The permutation
    (epoch_indices) and the identity of the draws -- (augment.seed, epoch, dataset row) -- are the same for all three
    tensors.  resident: the table on the device, two launches per batch (poses, frames); else the table in pinned memory,
    batches gathered into pinned staging and copied on a side stream `prefetch` batches ahead, the warp on the consumer's
    stream behind the copy's event.  transform_2d / transform_3d: as in PoseFeeder, on the pose outputs; frames are unchanged.
    crop: a PersonCrop: the batches are (frame, y1, y2, boxes).  Each frame is the person-centred square box of its row,
    taken from the row's source 2-D pose, resized to out_hw -- still the same two launches, each of which computes the box
    for itself from the same text; y1 is in crop coordinates ([0, 1] across the box), and so is what Model_2D learns to
    predict; boxes (b,4) fp32 = (x0, y0, side, side) in source pixels stays on the device.  Predictions go back to image
    coordinates with uncrop_poses(pred, boxes, frame_hw) (differentiable) before the lifter, the metrics or TriangleLoss see
    them, and a projector's output goes into crop coordinates with crop_poses; cycle_step itself knows nothing about crops --
    INTEGRATION.md has the wrapper that composes the two.  The streamed mode stages the batch's x2d rows beside its frames."""

    def __init__(self, frames, x2d, y3d, batch_size, *, out_hw=(256, 256), augment=None, device="cuda", shuffle=True,
                 seed=0, drop_last=False, rank=0, world=1, resident=True, prefetch=2, transform_2d=None, transform_3d=None,
                 crop=None):
        self._aug = _frame_augment_struct(augment)
        frames = torch.as_tensor(frames)
        self._code, self.out_hw, self._scale, self._fill = _frame_geometry(frames, out_hw, None, 0.0)
        self.crop = crop
        self._crop = _crop_struct(crop, frames.shape[1:3], augment)
        self.poses = PoseFeeder(x2d, y3d, batch_size, device=device, shuffle=shuffle, seed=seed, drop_last=drop_last,
                                rank=rank, world=world, resident=resident, prefetch=prefetch, augment=augment,
                                transform_2d=transform_2d, transform_3d=transform_3d, crop=crop,
                                frame_hw=frames.shape[1:3] if crop is not None else None)
        if frames.shape[0] != self.poses.n:
            raise ValueError("frames, x2d and y3d need the same number of rows")
        self.device, self.resident, self.prefetch = self.poses.device, resident, self.poses.prefetch
        frames = frames.contiguous()
        if resident:
            self.frames = frames.to(self.device)
        else:
            self.frames = frames.pin_memory()
            self._copy_stream = torch.cuda.Stream(self.device)

    def set_epoch(self, epoch):
        self.poses.set_epoch(epoch)

    def __len__(self):
        return len(self.poses)

    def __iter__(self):
        frames = self._iter_resident() if self.resident else self._iter_streamed()
        for frame, pose_batch in zip(frames, self.poses):      # (y1, y2), with a crop (y1, y2, boxes)
            yield (frame,) + tuple(pose_batch)

    def _warp(self, table, src_idx, row_ids, nb, epoch, x2d=None):
        out = torch.empty((nb,) + self.out_hw + (3,), dtype=torch.float32, device=self.device)
        with _lib.on_device(self.device):
            _frame_launch(table, self._code, src_idx, row_ids, nb, out, self._scale, self._fill, self._aug, epoch,
                          self._crop, x2d)
        return out

    def _iter_resident(self):
        batches, epoch = self.poses._indices(), self.poses.epoch
        if not batches:
            return
        sizes = [t.numel() for t in batches]
        idx_all = torch.cat(batches).to(self.device, non_blocking=True)
        at = 0
        for nb in sizes:                                  # the permutation slice is both the source frame and the draws' identity
            idx = idx_all[at:at + nb]
            at += nb
            yield self._warp(self.frames, idx, idx, nb, epoch, self.poses.a if self._crop is not None else None)

    def _iter_streamed(self):
        batches, epoch = self.poses._indices(), self.poses.epoch
        bs = self.poses.batch_size
        slots, inflight = self.prefetch + 1, []
        stage = [torch.empty((bs,) + tuple(self.frames.shape[1:]), dtype=self.frames.dtype).pin_memory() for _ in range(slots)]
        stage_idx = [torch.empty(bs, dtype=torch.int64).pin_memory() for _ in range(slots)]
        # a crop: the batch's source 2-D poses (136 B per frame) ride the same copy; the warp takes its boxes from them
        stage_x2d = [torch.empty(bs, self.poses.wa).pin_memory() for _ in range(slots)] if self._crop is not None else None
        free_events = [None] * slots                      # consumer done with the slot's previous batch

        def launch(k, idx):
            slot = k % slots
            nb = idx.numel()
            hf, hi = stage[slot][:nb], stage_idx[slot][:nb]
            if free_events[slot] is not None:
                free_events[slot].synchronize()           # staging buffer no longer being copied from
            torch.index_select(self.frames, 0, idx, out=hf)
            hi.copy_(idx)
            if stage_x2d is not None:
                hx = stage_x2d[slot][:nb]
                torch.index_select(self.poses.a, 0, idx, out=hx)
            with torch.cuda.stream(self._copy_stream):
                df = hf.to(self.device, non_blocking=True)
                di = hi.to(self.device, non_blocking=True)
                dx = hx.to(self.device, non_blocking=True) if stage_x2d is not None else None
                ev = torch.cuda.Event()
                ev.record(self._copy_stream)
            free_events[slot] = ev
            return df, di, dx, ev

        nxt = 0
        while nxt < len(batches) and len(inflight) < self.prefetch:
            inflight.append(launch(nxt, batches[nxt]))
            nxt += 1
        while inflight:
            df, di, dx, ev = inflight.pop(0)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            df.record_stream(cur)
            di.record_stream(cur)
            if dx is not None:
                dx.record_stream(cur)
            out = self._warp(df, None, di, di.numel(), epoch, dx)     # one launch on the consumer's stream, behind the event wait
            if nxt < len(batches):
                inflight.append(launch(nxt, batches[nxt]))
                nxt += 1
            yield out
