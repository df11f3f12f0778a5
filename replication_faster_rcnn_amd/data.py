"""Ground-truth data contract of the reference loader (utils/data_loader.py),
SURVEY.md §8(f) row 4.

The target creators (``targets``) and the training step consume gt exactly as
``voc_data`` produces it: ``box`` f64 [32, 4] in ``[ymin, xmin, ymax, xmax]``
order (row = height axis, the reference's "x"), rounded with ``np.around``,
rescaled to ``new_size``, every negative entry set to -1; ``label`` f64 [32]
with -1 for padding, difficult objects and unparsable objects.  Valid gt rows
are ``label != -1`` (train.py:74-76).

Host-side by nature (XML text, a few dozen numbers per image): the annotation
half of this module is the format, not a kernel.

The image half (utils/data_loader.py:38,61-75: ``skimage.transform.resize``,
``ToTensor``, ``Normalize``) runs on the device: ``pack_images`` lays a batch
of decoded uint8 images into one buffer and ``Preprocessor`` uploads it and
calls ``ops.preprocess`` / ``ops.rescale_boxes`` (DESIGN.md "Preprocessing").
Decoding the files (``skimage.io.imread``) stays with the caller.
"""
from __future__ import annotations

import xml.etree.ElementTree as ET

import numpy as np

from .utils import PASCAL_VOC_CLASSES, PASCAL_VOC_NUM_CLASSES

CLASS2NUM = dict(zip(PASCAL_VOC_CLASSES, range(PASCAL_VOC_NUM_CLASSES)))


def _etree_to_dict(el):
    """ElementTree -> the nested dict xmltodict.parse builds for a VOC
    annotation: leaves are text, a tag seen once is a dict, repeated tags a list."""
    children = list(el)
    if not children:
        return el.text
    out = {}
    for ch in children:
        v = _etree_to_dict(ch)
        if ch.tag in out:
            if not isinstance(out[ch.tag], list):
                out[ch.tag] = [out[ch.tag]]
            out[ch.tag].append(v)
        else:
            out[ch.tag] = v
    return out


def parse_voc_annotation(xml_text: str) -> dict:
    """xmltodict.parse(...) of a VOC annotation file (utils/data_loader.py:92)."""
    root = ET.fromstring(xml_text)
    return {root.tag: _etree_to_dict(root)}


def get_labels(doc: dict, difficult: bool = False, n_obj: int = 32, class2num=CLASS2NUM):
    """utils/data_loader.py:81-117 ``voc_data._get_labels`` on a parsed annotation.

    Kept as the reference behaves, quirks included (they decide which gt boxes
    the target creators see):
    * a single ``<object>`` parses to a dict, and the reference iterates its
      KEYS, so every row it touches becomes -1 (no valid gt for that image);
    * an unknown class name, a missing/unparsable bndbox or (with
      ``difficult=False``) a missing ``difficult`` tag marks the row -1;
    * boxes are ``np.around``-ed (half to even) AFTER parsing, -1 rows included.
    Returns (labels f64 [n_obj], boxes f64 [n_obj, 4]).
    """
    labels = -1 * np.ones(n_obj)
    boxes = -1 * np.ones([n_obj, 4])
    objects = doc["annotation"]["object"]
    for obj_ind, obj in enumerate(objects):
        if obj_ind >= n_obj:
            break
        try:
            labels[obj_ind] = class2num[obj["name"]]
            bb = obj["bndbox"]
            boxes[obj_ind, :] = np.array([float(bb["ymin"]), float(bb["xmin"]),
                                          float(bb["ymax"]), float(bb["xmax"])])
            if not difficult and obj["difficult"] == "1":
                labels[obj_ind] = -1
        except Exception:  # the reference's bare except (utils/data_loader.py:112)
            labels[obj_ind] = -1
            boxes[obj_ind, :] = [-1, -1, -1, -1]
    return np.array(labels), np.around(boxes)


def get_difficult(doc: dict, n_obj: int = 32, class2num=CLASS2NUM) -> np.ndarray:
    """The ``difficult`` flag ``voc_data._get_labels`` (utils/data_loader.py:81-117)
    folds into ``label = -1`` or drops, kept for the evaluator: uint8 [n_obj], 1
    where that object's ``difficult`` tag is ``"1"``.  Rows line up with
    ``get_labels(doc, difficult=True)``; a row that call marks -1 (unknown class,
    unparsable bndbox, the single-``<object>`` quirk, padding) is 0."""
    flags = np.zeros(n_obj, np.uint8)
    objects = doc["annotation"]["object"]
    for obj_ind, obj in enumerate(objects):
        if obj_ind >= n_obj:
            break
        try:
            class2num[obj["name"]]
            bb = obj["bndbox"]
            [float(bb[k]) for k in ("ymin", "xmin", "ymax", "xmax")]
            flags[obj_ind] = 1 if obj.get("difficult") == "1" else 0
        except Exception:  # the rows get_labels' bare except marks -1
            flags[obj_ind] = 0
    return flags


def rescale_boxes(box: np.ndarray, image_hw, new_size=(600, 600)) -> np.ndarray:
    """utils/data_loader.py:63-70: rows (cols 0,2) by image height, cols 1,3 by
    width, in f64 (divide, then multiply); negative entries -> -1.  Returns a
    new array (the reference edits in place)."""
    b = np.array(box, dtype=np.float64, copy=True)
    new_h, new_w = new_size
    b[:, [0, 2]] = b[:, [0, 2]] / image_hw[0] * new_h
    b[:, [1, 3]] = b[:, [1, 3]] / image_hw[1] * new_w
    b[b < 0] = -1
    return b


def load_targets(xml_text: str, image_hw, new_size=(600, 600), difficult=False, n_obj=32,
                 return_difficult=False):
    """One ``voc_data.__getitem__``'s (box, label) pair (image handling aside).
    With ``return_difficult`` also ``get_difficult``'s flags: (box, label,
    difficult) -- an evaluator wants ``difficult=True`` with it, so that the
    difficult objects stay in as gt rows."""
    doc = parse_voc_annotation(xml_text)
    label, box = get_labels(doc, difficult=difficult, n_obj=n_obj)
    if return_difficult:
        return rescale_boxes(box, image_hw, new_size), label, get_difficult(doc, n_obj=n_obj)
    return rescale_boxes(box, image_hw, new_size), label


def collate_targets(samples):
    """DataLoader default collate of the (box, label) pairs -> the batch
    tensors train.py:59-76 indexes: box [N, 32, 4] f64, label [N, 32] f64."""
    import torch
    boxes = torch.from_numpy(np.stack([s[0] for s in samples]))
    labels = torch.from_numpy(np.stack([s[1] for s in samples]))
    return boxes, labels


def pack_images(images):
    """A batch of decoded images -> the inputs of ``ops.preprocess``, on the host.

    ``images``: a list of H x W x 3 uint8 numpy arrays or torch tensors (RGB, any
    strides, sizes may differ).  Anything else -- grayscale, RGBA, another dtype,
    an empty image -- is rejected with a ValueError naming the image: they are
    outside the contract, as they are for the reference.  Returns (pixels uint8
    [B] with the images back to back in list order, pinned when a device is
    present; offset int64 [N]; hw int32 [N, 2]; (max h, max w)), the first three
    host tensors ready for a non-blocking upload."""
    import torch
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError("pack_images: images must be a non-empty list of H x W x 3 uint8 arrays")
    arrs = []
    for i, im in enumerate(images):
        if isinstance(im, torch.Tensor):
            if im.dtype != torch.uint8:
                raise ValueError(f"pack_images: image {i} has dtype {im.dtype}; must be uint8")
            im = im.detach().cpu().numpy()
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8:
            got = f"dtype {im.dtype}" if isinstance(im, np.ndarray) else type(im).__name__
            raise ValueError(f"pack_images: image {i} must be a uint8 numpy array or tensor; got {got}")
        if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError(f"pack_images: image {i} has shape {tuple(im.shape)}; must be H x W x 3 (RGB) "
                             "with H, W >= 1")
        arrs.append(im)
    hw = np.array([a.shape[:2] for a in arrs], np.int32)
    sizes = 3 * hw[:, 0].astype(np.int64) * hw[:, 1]
    offset = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pixels = torch.empty(int(sizes.sum()), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    flat = pixels.numpy()
    for a, o, s in zip(arrs, offset, sizes):
        flat[o:o + s] = a.reshape(-1)
    return pixels, torch.from_numpy(offset), torch.from_numpy(hw), (int(hw[:, 0].max()), int(hw[:, 1].max()))


class Preprocessor:
    """``voc_data.__getitem__``'s image branch (utils/data_loader.py:61-75) for a
    batch, on the device: ``pack_images``, one upload, ``ops.preprocess`` and,
    with boxes, ``ops.rescale_boxes``.

    ``Preprocessor(new_size)(images, boxes=None)`` -> (image fp32 [N, 3, H, W],
    boxes fp64 [N, G, 4] or None, hw int32 [N, 2]), all on the device with no
    synchronisation: what ``Trainer.train_step`` and ``FasterRCNN.predict`` take
    as they are.  ``boxes``: [N, G, 4] in each image's own pixels, as
    ``get_labels`` returns them (numpy or tensor).  ``self.status`` keeps the
    last call's int32 [N] status (device; 0 = ok) for whoever wants to read it."""

    def __init__(self, new_size=(600, 600), mean=None, std=None):
        self.new_size = (int(new_size[0]), int(new_size[1]))
        self.mean, self.std = mean, std
        self.status = None

    def __call__(self, images, boxes=None):
        import torch
        from . import _lib, ops
        pixels, offset, hw, max_hw = pack_images(images)
        dev = _lib.device()
        pixels, offset, hw = (t.to(dev, non_blocking=True) for t in (pixels, offset, hw))
        kw = {}
        if self.mean is not None:
            kw["mean"] = self.mean
        if self.std is not None:
            kw["std"] = self.std
        image, self.status = ops.preprocess(pixels, offset, hw, self.new_size, max_hw=max_hw, **kw)
        if boxes is not None:
            b = torch.as_tensor(np.asarray(boxes) if not isinstance(boxes, torch.Tensor) else boxes)
            if b.dim() != 3 or b.shape[0] != len(images) or b.shape[2] != 4:
                raise ValueError(f"Preprocessor: boxes must be [N={len(images)}, G, 4]; got {tuple(b.shape)}")
            boxes = ops.rescale_boxes(b.to(dev, torch.float64).contiguous(), hw, self.new_size)
        return image, boxes, hw
