"""Model inputs built on the MI355X (csrc/resize.hip, data.prepare_batch, data.ImageFolderLoader): the device
resize equals PIL.Image.resize bit for bit, its f32 forms equal torch's ToTensor / Normalize bitwise, the device
grayscale equals scores.imread_gray's formula, and the loader yields what the host path (testing.load_test_images,
scores.preprocess_image_scores) yields.  Every comparison is equality."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def pil_resize(a, hw, filt="bicubic"):
    """uint8 [n][H][W][3] -> [n][h][w][3] through PIL, one image at a time"""
    return np.stack([np.array(Image.fromarray(x).resize((hw[1], hw[0]), FILTERS[filt])) for x in a])


def blocks(H, W):
    """hard-edged blocks: thousands of the horizontal sums overshoot below 0 and above 255, so both clips run"""
    y, x = np.mgrid[0:H, 0:W]
    a = (255 * (((y // 5) + (x // 7)) % 2)).astype(np.uint8)
    return np.stack([a, 255 - a, a], axis=-1)


def rand(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


# name, source [n][H][W][3], output (h, w)
CASES = [
    ("kodak-down", rand(1, 512, 768, 1), (224, 224)),
    ("odd-width-53-up", rand(1, 37, 53, 2), (224, 224)),
    ("up-both", rand(1, 224, 224, 3), (512, 768)),
    ("wide-taps-73-up-rows", rand(1, 100, 300, 4), (333, 17)),        # 300 -> 17 columns, 100 -> 333 rows
    ("skip-both", rand(2, 16, 16, 5), (16, 16)),
    ("single-row", rand(1, 1, 5, 6), (3, 7)),
    ("batch-stride", rand(3, 37, 53, 7), (29, 31)),
    ("clip-32", blocks(45, 77)[None], (32, 32)),
    ("clip-up", blocks(45, 77)[None], (96, 160)),                     # both axes up; odd width 77
    ("wide-taps-33", rand(1, 4, 2040, 8), (4, 256)),                  # vertical pass skipped
    ("skip-horizontal", rand(2, 40, 24, 9), (13, 24)),
    ("down-rows-up-cols", rand(1, 90, 20, 10), (30, 61)),
    ("one-output", rand(1, 9, 11, 11), (1, 1)),
]


@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("name,src,hw", CASES, ids=[c[0] for c in CASES])
def test_resize_u8_equals_pil(tmae, name, src, hw, filt):
    got = tmae.ops.resize_u8(torch.from_numpy(src).to(DEV), hw, filter=filt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (src.shape[0], hw[0], hw[1], 3)
    np.testing.assert_array_equal(got.cpu().numpy(), pil_resize(src, hw, filt))


def test_clip_case_overshoots_both_ways(tmae):
    """the block image drives the unclipped horizontal sums outside 0..255 on both sides (what the two clip
    cases above rely on)"""
    a = blocks(45, 77).astype(np.int64)
    kk, bounds = tmae.ops.resize_tables(77, 32)
    acc = np.stack([(1 << 21) + a[:, x0:x0 + n, 0] @ kk[xo, :n].astype(np.int64) for xo, (x0, n) in enumerate(bounds)])
    assert ((acc >> 22) < 0).sum() > 100 and ((acc >> 22) > 255).sum() > 100


def test_resize_u8_unaligned_view(tmae):
    """a batch that starts at an odd byte address: the staged rows keep their own misalignment"""
    src = rand(2, 21, 35, 12)
    flat = torch.zeros(src.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(src).to(DEV).flatten()
    view = flat[1:].view(2, 21, 35, 3)
    assert view.data_ptr() % 4 == 1
    np.testing.assert_array_equal(tmae.ops.resize_u8(view, (10, 12)).cpu().numpy(), pil_resize(src, (10, 12)))
    gray = tmae.ops.rgb_to_gray_u8(view).cpu().numpy()
    np.testing.assert_array_equal(gray, gray_host(src))


def test_resize_u8_single_image(tmae):
    src = rand(1, 33, 47, 13)
    got = tmae.ops.resize_u8(torch.from_numpy(src[0]).to(DEV), 24)
    np.testing.assert_array_equal(got.cpu().numpy(), pil_resize(src, (24, 24))[0])


@pytest.mark.parametrize("name,src,hw", [CASES[1], CASES[4], CASES[6], CASES[9], CASES[10]],
                         ids=["two-pass", "skip-both", "batch", "horizontal-only", "vertical-only"])
def test_resize_f32_bitwise_torch(tmae, name, src, hw):
    """ToTensor (/ 255) and Normalize (sub mean, div std) as torch computes them from PIL's uint8 result"""
    u8 = torch.from_numpy(pil_resize(src, hw)).permute(0, 3, 1, 2)
    dev = torch.from_numpy(src).to(DEV)
    plain = tmae.ops.resize_u8(dev, hw, out="f32")
    assert plain.dtype == torch.float32 and tuple(plain.shape) == (src.shape[0], 3, hw[0], hw[1])
    assert torch.equal(plain.cpu(), u8.float() / 255)
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    norm = tmae.ops.resize_u8(dev, hw, out="f32", mean=MEAN, std=STD)
    assert torch.equal(norm.cpu(), (u8.float() / 255 - m) / s)


def test_resize_u8_rejects_bad_arguments(tmae):
    x = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        tmae.ops.resize_u8(x.float(), 2)
    with pytest.raises(ValueError):
        tmae.ops.resize_u8(x, 0)
    with pytest.raises(ValueError):
        tmae.ops.resize_u8(x, 2, out="u8", mean=MEAN, std=STD)
    with pytest.raises(ValueError):
        tmae.ops.resize_u8(x[..., :2], 2)


def gray_host(rgb):
    v = rgb.astype(np.int64)
    return ((9798 * v[..., 0] + 19235 * v[..., 1] + 3735 * v[..., 2] + 16384) >> 15).astype(np.uint8)


def test_rgb_to_gray_u8(tmae):
    src = rand(3, 37, 53, 20)           # 5883 pixels: groups of four and a tail of three
    src[1] = 0
    src[2] = 255
    src[0, :8] = np.random.default_rng(21).choice(np.array([0, 255], dtype=np.uint8), (8, 53, 3))
    got = tmae.ops.rgb_to_gray_u8(torch.from_numpy(src).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 37, 53)
    np.testing.assert_array_equal(got.cpu().numpy(), gray_host(src))
    one = tmae.ops.rgb_to_gray_u8(torch.from_numpy(src[0, 0, :3]).to(DEV))  # fewer than four pixels
    np.testing.assert_array_equal(one.cpu().numpy(), gray_host(src[0, 0, :3]))


def test_prepare_batch(tmae):
    from textmae_amd.data import prepare_batch
    from textmae_amd.scores import image_scores

    src = rand(3, 70, 101, 30)
    src[1, :40] = 100                    # a flat region: the quadtree merges it
    ref_scores = image_scores(torch.from_numpy(gray_host(src)).to(DEV), 64, 16)
    u8 = torch.from_numpy(pil_resize(src, (64, 64))).permute(0, 3, 1, 2)
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    imgs, sc = prepare_batch(src, size=64, patch=16)               # a host batch: one upload
    assert imgs.is_cuda and sc.is_cuda and tuple(sc.shape) == (3, 16)
    assert torch.equal(imgs.cpu(), (u8.float() / 255 - m) / s)
    assert torch.equal(sc, ref_scores)
    imgs, sc = prepare_batch(torch.from_numpy(src).to(DEV), size=64, normalize=False, scores=False)
    assert sc is None and torch.equal(imgs.cpu(), u8.float() / 255)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """five PNGs of two shapes in each of two datasets: <base>/flat/*.png (the test layout: the dataset folder
    itself) and <base>/split/train/*.png (the train layout)"""
    base = tmp_path_factory.mktemp("images")
    (base / "flat").mkdir()
    (base / "split" / "train").mkdir(parents=True)
    shapes = [(48, 80), (60, 40), (48, 80), (60, 40), (48, 80)]
    for i, (h, w) in enumerate(shapes):
        a = rand(1, h, w, 40 + i)[0]
        a[: h // 2, : w // 2] = 90 + 10 * i   # structure for the score producer
        Image.fromarray(a).save(base / "flat" / f"img{i}.png")
        Image.fromarray(a[::-1].copy()).save(base / "split" / "train" / f"t{i}.png")
    return base, shapes


def test_image_folder_loader_test_mode(tmae, folder):
    from textmae_amd.data import ImageFolderLoader
    from textmae_amd.scores import preprocess_image_scores
    from textmae_amd.testing import load_test_images

    base, shapes = folder
    root = base / "flat"
    paths = sorted(root.glob("*.png"))
    host = load_test_images(paths, 64)
    ref_scores = preprocess_image_scores(paths, 64)
    loader = ImageFolderLoader(root, "test", batch_size=2, size=64)
    assert len(loader) == 3 and [p.name for p in loader.imgs_path] == [p.name for p in paths]
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [2, 2, 1]   # the last short batch is yielded
    imgs = torch.cat([b[0] for b in batches]).cpu()
    ori = [o for b in batches for o in b[1]]
    sc = torch.cat([b[2] for b in batches]).cpu()
    assert all(b[0].is_cuda and b[2].is_cuda for b in batches)
    assert ori == [(w, h) for h, w in shapes] == [o for _, o in host]
    assert torch.equal(imgs, torch.cat([x for x, _ in host]))
    assert torch.equal(sc, ref_scores)
    assert len(list(ImageFolderLoader(root, "test", batch_size=2, size=64, drop_last=True))) == 2


def test_image_folder_loader_train_mode(tmae, folder):
    from textmae_amd.data import ImageFolderLoader
    from textmae_amd.scores import preprocess_image_scores
    from textmae_amd.testing import load_test_images

    base, shapes = folder
    root = base / "split"
    paths = sorted((root / "train").glob("*.png"))
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    host = (torch.cat([x for x, _ in load_test_images(paths, 64)]) - m) / s
    ref_scores = preprocess_image_scores(paths, 64)
    imgs, ori, sc = next(iter(ImageFolderLoader(root, "train", batch_size=5, size=64)))   # both shapes in one batch
    assert ori == [(w, h) for h, w in shapes]
    assert torch.equal(imgs.cpu(), host)
    assert torch.equal(sc.cpu(), ref_scores)
    # a shuffled epoch is a permutation of the same samples, the same for one seed
    a = list(ImageFolderLoader(root, "train", batch_size=5, size=64, shuffle=True, seed=3))[0]
    b = list(ImageFolderLoader(root, "train", batch_size=5, size=64, shuffle=True, seed=3))[0]
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert sorted(x.flatten().tolist() for x in a[2].cpu()) == sorted(x.flatten().tolist() for x in sc.cpu())


def test_image_folder_loader_jpeg_gray_from_host(tmae, tmp_path):
    """a JPEG's grayscale stays the host's imread_gray (libjpeg's luma plane), also for the PNG sharing its group"""
    from textmae_amd.data import ImageFolderLoader
    from textmae_amd.scores import preprocess_image_scores
    from textmae_amd.testing import load_test_images

    ds = tmp_path / "mixed"
    ds.mkdir()
    a = rand(2, 48, 80, 60)
    a[:, :24, :40] = 120
    Image.fromarray(a[0]).save(ds / "a.jpg", quality=90)
    Image.fromarray(a[1]).save(ds / "b.png")
    paths = sorted(ds.glob("*.*"))
    imgs, ori, sc = next(iter(ImageFolderLoader(ds, "test", batch_size=2, size=64)))
    assert ori == [(80, 48), (80, 48)]
    assert torch.equal(imgs.cpu(), torch.cat([x for x, _ in load_test_images(paths, 64)]))
    assert torch.equal(sc.cpu(), preprocess_image_scores(paths, 64))


def test_image_folder_loader_reads_score_file(tmae, folder, tmp_path):
    """<dataset>_scores/<mode>.pt, indexed by sorted position, replaces the device producer"""
    import shutil

    from textmae_amd.data import ImageFolderLoader

    base, _ = folder
    ds = tmp_path / "copy"
    shutil.copytree(base / "flat", ds)
    (tmp_path / "copy_scores").mkdir()
    saved = torch.rand(5, 16, generator=torch.Generator().manual_seed(1))
    torch.save(saved, tmp_path / "copy_scores" / "test.pt")
    got = torch.cat([b[2] for b in ImageFolderLoader(ds, "test", batch_size=3, size=64)])
    assert torch.equal(got.cpu(), saved)


def test_train_one_epoch_accepts_the_loader(tmae, folder):
    from test_gpu_optim_dp import SMALL, _model
    from textmae_amd import engine
    from textmae_amd.data import ImageFolderLoader
    from textmae_amd.optim import configure_optimizers
    from textmae_amd.rd_loss import RateDistortionLoss

    root = folder[0] / "split"
    m, cfg = _model(SMALL, 21, torch.float32)
    m.distortion = "ssim+l1"
    opt, aux = configure_optimizers(m, lr=1e-3, aux_lr=1e-3, fused=True)
    loader = ImageFolderLoader(root, "train", batch_size=5, size=cfg.img_size, patch=cfg.patch_size)
    stats = engine.train_one_epoch(m, RateDistortionLoss(lmbda=1e-2), loader, opt, aux, epoch=0)
    assert set(stats) == set(engine.METRICS) and all(np.isfinite(v) for v in stats.values())


def test_load_test_images_on_device(tmae, folder):
    from textmae_amd.testing import load_test_images

    paths = sorted((folder[0] / "flat").glob("*.png"))
    host = load_test_images(paths, 64)
    dev = load_test_images(paths, 64, device=DEV)
    for (a, oa), (b, ob) in zip(host, dev):
        assert b.is_cuda and oa == ob and torch.equal(a, b.cpu())


def test_save_output_original_size(tmae, tmp_path):
    from textmae_amd.testing import save_output

    x = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(2)) * 1.2 - 0.1
    u8 = x.squeeze().clamp(0, 1).mul(255).round().byte().permute(1, 2, 0).numpy()
    save_output(x.to(DEV), (301, 173), "full.png", str(tmp_path), original_size=True)
    got = Image.open(tmp_path / "full.png")
    assert got.size == (301, 173)
    np.testing.assert_array_equal(np.array(got), np.array(Image.fromarray(u8).resize((301, 173), Image.BICUBIC)))
    save_output(x.to(DEV), (301, 173), "plain.png", str(tmp_path))   # the default keeps the 224^2 output
    np.testing.assert_array_equal(np.array(Image.open(tmp_path / "plain.png")), u8)
