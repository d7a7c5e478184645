"""Model inputs: the image-folder loader of the reference (utils/dataloader.py) with its per-sample transform
on the device, and the synthetic DIV2K-shaped training set of the benchmark.

``prepare_batch`` / ``ImageFolderLoader``: the reference feeds the model through ``get_image_dataset``
(utils/dataloader.py:47-78): ``Image.open().convert("RGB")``, ``transforms.Resize((224, 224), BICUBIC)`` on the
PIL image, ``ToTensor`` and, for train / val, ``Normalize``.  Here the decode stays on the host and everything
after it runs on the device from one uint8 upload per group of equally shaped images: the Pillow-exact resize
with the ToTensor / Normalize epilogue (``ops.resize_u8``), the grayscale conversion and the score-map producer
(``ops.rgb_to_gray_u8``, ``scores.image_scores``).

``SyntheticCropSet``: synthetic DIV2K-shaped training set for the data-parallel training step (BASELINE config 3,
SURVEY §8(d)).

The reference trains from an image folder through ``get_image_dataset`` (utils/dataloader.py:47-78)
and a ``DistributedSampler`` (training.py:122-129), seeding each process with ``args.seed + rank``
(training.py:109-110).  There is no network here, so config 3 stands in DIV2K's shape: per rank, a
few seeded uint8 noise images of 2040 x 1356 (DIV2K's landscape size), kept resident in HBM, and every
sample is a random 256 x 256 crop of one of them, converted like the loader's ToTensor + Normalize
(dataloader.py:58-61) by one device kernel (``ops.crop_normalize_u8``).  Crop positions and patch
scores are drawn up front from a host generator seeded with ``seed + rank``, so the timed steps do
no host work and no host synchronisation.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import ops

DIV2K_HW = (1356, 2040)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class SyntheticCropSet:
    def __init__(self, device, seed: int, rank: int = 0, num_images: int = 16, crop: int = 256,
                 patch_size: int = 16, hw=DIV2K_HW):
        self.device = torch.device(device)
        self.crop, self.hw = crop, hw
        self.L = (crop // patch_size) ** 2
        self.gen = torch.Generator().manual_seed(seed + rank)
        H, W = hw
        src = torch.randint(0, 256, (num_images, H, W, 3), dtype=torch.uint8, generator=self.gen)
        self.images = src.to(self.device)
        self._plan = None
        self._i = 0

    def plan(self, steps: int, batch: int):
        """draw `steps` batches of (image, top, left) crops and patch scores; uploaded once"""
        H, W = self.hw
        n = self.images.shape[0]
        c = torch.stack([torch.randint(0, n, (steps, batch), generator=self.gen),
                         torch.randint(0, H - self.crop + 1, (steps, batch), generator=self.gen),
                         torch.randint(0, W - self.crop + 1, (steps, batch), generator=self.gen)], dim=-1)
        scores = torch.rand(steps, batch, self.L, generator=self.gen)
        self._plan = (c.to(torch.int32).to(self.device), scores.to(self.device))
        self._i = 0
        self._out = [torch.empty((batch, 3, self.crop, self.crop), dtype=torch.float32, device=self.device)
                     for _ in range(2)]
        return self

    def next(self):
        """the next planned batch: (imgs [B, 3, crop, crop] f32 normalised, total_scores [B, L] f32)"""
        crops, scores = self._plan
        n = self._i
        self._i += 1
        i = n % crops.shape[0]
        # two buffers, alternating on the monotonic call count (not the wrapped plan index, which repeats a
        # buffer when an odd-length plan wraps): a batch stays valid while the next one is cut
        out = self._out[n & 1]
        ops.crop_normalize_u8(self.images, crops[i], self.crop, IMAGENET_MEAN, IMAGENET_STD, out=out)
        return out, scores[i]


def prepare_batch(rgb_u8, size: int = 224, patch: int = 16, normalize: bool = True, scores: bool = True,
                  device="cuda"):
    """One batch of decoded images into model inputs, on the device.

    rgb_u8: uint8 [n, H, W, 3] (numpy array or tensor; a host batch is uploaded once, as uint8).  Returns
    ``(imgs, total_scores)``: imgs f32 [n, 3, size, size] = ToTensor(PIL bicubic resize), with the ImageNet
    Normalize when ``normalize`` (train / val; the test transform has none); total_scores f32 [n, (size / patch)^2]
    = ``image_scores`` of the images' grayscale (``None`` when ``scores`` is off)."""
    from .scores import image_scores

    x = torch.from_numpy(np.ascontiguousarray(rgb_u8)) if isinstance(rgb_u8, np.ndarray) else rgb_u8
    if x.dim() != 4 or x.shape[3] != 3 or x.dtype != torch.uint8:
        raise ValueError(f"prepare_batch needs uint8 [n, H, W, 3], got {x.dtype} {tuple(x.shape)}")
    if not x.is_cuda:
        x = x.to(device)
    x = x.contiguous()
    if normalize:
        imgs = ops.resize_u8(x, size, out="f32", mean=IMAGENET_MEAN, std=IMAGENET_STD)
    else:
        imgs = ops.resize_u8(x, size, out="f32")
    total_scores = image_scores(ops.rgb_to_gray_u8(x), size, patch) if scores else None
    return imgs, total_scores


class ImageFolderLoader:
    """``get_image_dataset(mode, dataset_path)`` behind a batch loader (utils/dataloader.py:12-78, training.py:115-129):
    images from ``dataset_path`` (test) or ``dataset_path/mode`` (train / val) in sorted order, resized to
    ``size`` x ``size`` like the reference transform, ImageNet-normalised for train / val.  Iterates
    ``(imgs [B, 3, size, size] f32 on the device, ori_shapes, total_scores [B, L] f32 on the device)`` -- the triple
    engine.train_one_epoch / val_one_epoch consume; ori_shapes is the list of PIL ``(W, H)`` sizes.

    The host decodes (``Image.open().convert("RGB")``); images of one shape inside a batch go to the device in one
    uint8 upload and one ``prepare_batch`` call, the batch comes out in input order.  Scores are read from
    ``<dataset>_scores/<mode>.pt`` when that file exists (indexed by the sorted position, as the reference dataset
    does), otherwise they come from the device producer.  For JPEG files the producer's grayscale keeps coming from
    the host ``imread_gray`` (libjpeg's luma plane, not the RGB formula)."""

    def __init__(self, dataset_path, mode: str, batch_size: int, size: int = 224, device="cuda", shuffle: bool = False,
                 seed: int = 0, drop_last: bool = False, patch: int = 16):
        from .scores import IMG_EXTENSIONS

        if mode not in ("train", "val", "test"):
            raise ValueError("Mode must be one of ['train', 'val', 'test']")
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.dataset_path = Path(dataset_path)
        self.mode, self.batch_size, self.size, self.patch = mode, int(batch_size), int(size), int(patch)
        self.device = torch.device(device)
        self.shuffle, self.seed, self.drop_last = shuffle, seed, drop_last
        self.normalize = mode != "test"
        self.root = self.dataset_path if mode == "test" else self.dataset_path / mode
        self.imgs_path = sorted(p for p in self.root.rglob("*.*") if p.suffix.lower() in IMG_EXTENSIONS)
        if not self.imgs_path:
            raise ValueError(f"No images found in {self.root}")
        score_file = self.dataset_path.parent / f"{self.dataset_path.name}_scores" / f"{mode}.pt"
        self.scores = None
        if score_file.exists():
            self.scores = torch.load(score_file, map_location="cpu", weights_only=True)
            if len(self.scores) != len(self.imgs_path):
                raise ValueError(f"{score_file} holds {len(self.scores)} score rows for {len(self.imgs_path)} images")
        self._epochs = 0  # iterations started: a shuffled epoch is seeded with seed + this count

    def __len__(self):
        n = len(self.imgs_path)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _order(self):
        n = len(self.imgs_path)
        epoch, self._epochs = self._epochs, self._epochs + 1
        if not self.shuffle:
            return list(range(n))
        g = torch.Generator().manual_seed(self.seed + epoch)
        return torch.randperm(n, generator=g).tolist()

    def _load(self, idx):
        from PIL import Image

        from .scores import image_scores, imread_gray

        S, L = self.size, (self.size // self.patch) ** 2
        decoded, ori_shapes, jpeg = [], [], []
        for i in idx:
            with Image.open(self.imgs_path[i]) as im:
                jpeg.append(im.format == "JPEG")
                rgb = im.convert("RGB")
            ori_shapes.append(rgb.size)
            decoded.append(np.asarray(rgb))
        B = len(idx)
        imgs = torch.empty((B, 3, S, S), dtype=torch.float32, device=self.device)
        total_scores = torch.empty((B, L), dtype=torch.float32, device=self.device)
        by_shape = {}
        for j, a in enumerate(decoded):
            by_shape.setdefault(a.shape, []).append(j)
        need_scores = self.scores is None
        for members in by_shape.values():
            at = torch.tensor(members, device=self.device)
            batch = np.stack([decoded[j] for j in members])
            device_gray = need_scores and not any(jpeg[j] for j in members)
            x, sc = prepare_batch(batch, S, self.patch, self.normalize, device_gray, self.device)
            imgs.index_copy_(0, at, x)
            if need_scores and not device_gray:  # a group with JPEG files: the host grayscale for all of it
                gray = np.stack([imread_gray(self.imgs_path[idx[j]]) for j in members])
                sc = image_scores(torch.from_numpy(gray).to(self.device), S, self.patch)
            if need_scores:
                total_scores.index_copy_(0, at, sc)
        if not need_scores:
            total_scores.copy_(self.scores[torch.tensor(idx)].to(torch.float32))
        return imgs, ori_shapes, total_scores

    def __iter__(self):
        order = self._order()
        for s in range(0, len(order), self.batch_size):
            idx = order[s:s + self.batch_size]
            if len(idx) < self.batch_size and self.drop_last:
                return
            yield self._load(idx)
