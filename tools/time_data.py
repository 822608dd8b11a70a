"""The input pipeline (locov_amd/data.py): DatasetMapper.map_batch on the device against its own host path and, where Pillow imports,
against Pillow on the same machine; and the resize kernel alone.

    timeout -k 10 600 python tools/time_data.py [--images 1 8] [--iters 50] [--warmup 10] [--threads 16] [--out records.json]
    timeout -k 10 600 python tools/time_data.py --proposals 1000 --images 1 8 32      (the proposal side instead: proposals() below)
    timeout -k 10 600 python tools/time_data.py --strong --images 8                   (the strong augmentation instead: strong() below)
    timeout -k 10 900 python tools/time_data.py --jpeg --images 8                     (the mapper from JPEG files instead: jpeg() below)

For each source size (480 x 640 and 3000 x 4000, both to 800 x 1067: INPUT.MIN_SIZE_TEST 800, MAX_SIZE_TEST 1333) and batch size:
  (a) kernel     ops.resize_flip_images on images already on the device: device-event time per call, the kernel's device time
                 (torch.profiler: the event time of so short a call is mostly the host's) and its bytes per second -- the
                 algorithmic traffic, source bytes read once + output bytes written -- beside the measured copy rate --copy-tbs.
  (b) map_batch  host wall time from numpy HWC images to the dicts, the image on the device at the end of every side:
                   device   DatasetMapper(device="cuda"): upload of the raw bytes, one launch
                   host     DatasetMapper(device="cpu") (this module's numpy definition, one thread), then .to(device)
                   pillow   Image.fromarray(img).resize(..., BILINEAR), transposed, then .to(device): on one thread, and on a pool of
                            --threads threads (Pillow releases the GIL while it resamples), at most one image per thread
Protocol: >= 10 warm-up and >= 50 timed iterations for the device sides; the slow host sides run --host-iters times.
Medians with 10th / 90th percentiles.  Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_backbone import alternate, kernels  # noqa: E402  (tools/ is the script directory)
from time_detector import wall  # noqa: E402

SOURCES = [(480, 640), (3000, 4000)]


class _Metadata:
    thing_classes = [f"class {i}" for i in range(80)]

    def __init__(self, **entries):
        self.entries = entries

    def get(self, name, default=None):
        return self.entries.get(name, default)


def proposals(args, dev):
    """--proposals N: CocoImageDatasetMapper.map_batch (training, MODEL.LOAD_OBJ_PROPOSALS) on 480 x 640 images with N fp32
    proposals each, the three sides alternating in one process -- host wall time to the synchronised dicts:
        fused     LOCOV_FUSED_PROPOSALS=1: the store's rows stay on the device, one descriptor and one launch per batch
        host      LOCOV_FUSED_PROPOSALS=0: data.py's numpy / torch definition per image, its result moved to the device
        no_proposals   the same mapper without object_proposals in its metadata (what the image and annotation side costs)
    and ops.map_proposals alone: device-event time per call and the launch's own device time (torch.profiler)."""
    import locov_amd
    from locov_amd import data, ops
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.DEVICE, cfg.MODEL.LOAD_OBJ_PROPOSALS = str(dev), True
    h, w, n_rows = 480, 640, int(args.proposals)
    rec = {"device": torch.cuda.get_device_name(dev), "proposals_per_image": n_rows, "source": [h, w], "runs": {}}
    for N in args.images:
        rng = np.random.default_rng(N)
        x1, y1 = rng.uniform(-20, w, (2, N, n_rows))
        rows = np.stack([x1, y1, x1 + rng.uniform(-5, 300, (N, n_rows)), y1 + rng.uniform(-5, 300, (N, n_rows)),
                         rng.uniform(0.3, 1.0, (N, n_rows))], axis=2).astype(np.float32)
        dicts = [{"image_raw": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "image_id": i,
                  "annotations": [{"bbox": [10.0 * k, 20.0, 100.0, 80.0], "bbox_mode": data.XYWH_ABS, "category_id": k} for k in range(7)]}
                 for i in range(N)]
        captions = {i: ["a caption", "another caption"] for i in range(N)}
        with_store = data.CocoImageDatasetMapper(cfg, _Metadata(captions_dict=captions, object_proposals={i: rows[i] for i in range(N)}), True,
                                                 device=dev, seed=1)
        without = data.CocoImageDatasetMapper(cfg, _Metadata(captions_dict=captions), True, device=dev, seed=1)
        sample = with_store.draw_sample(dicts)

        def side(mapper, fused):
            def step():
                os.environ["LOCOV_FUSED_PROPOSALS"] = fused
                return mapper.map_batch(dicts, sample)
            return step

        sides = {"fused": side(with_store, "1"), "host": side(with_store, "0"), "no_proposals": side(without, "1")}
        for a, b in zip(sides["fused"](), sides["host"]()):
            assert torch.equal(a["instances"].gt_boxes.tensor, b["instances"].gt_boxes.tensor), "the device path and the definition differ"
        ms = {k: [] for k in sides}
        names = list(sides)
        for it in range(args.warmup + args.iters):
            for k in (names if it % 2 == 0 else names[::-1]):
                t = wall(sides[k], 1, 0)
                if it >= args.warmup:
                    ms[k].append(t["median_ms"])
        size = data.ResizeShortestEdge.get_output_shape(h, w, 800, 1333)
        table = [with_store.store.table[i] for i in range(N)]
        launch = lambda: ops.map_proposals(with_store.store.rows, [s for s, _ in table], [n for _, n in table], [(size[1] / w, size[0] / h)] * N,
                                           [int(f) for f in sample["flip"]], [size] * N, cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN, data.OBJECTNESS_THR)
        r = {"map_batch": {k: {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
                           for k, v in ms.items()},
             "pseudo_gt_per_image": [len(d["instances"]) for d in sides["fused"]()][:4],
             "map_proposals": dict(alternate({"call": launch}, args.iters, args.warmup)["call"], device=kernels(launch, top=2))}
        rec["runs"][f"images_{N}"] = r
        print(json.dumps({f"proposals {n_rows} images {N}": r}), flush=True)
    os.environ.pop("LOCOV_FUSED_PROPOSALS", None)
    return rec


STRONG_GROUPS = {"all": dict(COLOR_JITTER=0.4, RANDOM_GRAY_SCALE=True, GAUSSIAN_BLUR=True, RANDOM_ERASE=True),
                 "blur": dict(GAUSSIAN_BLUR=True), "jitter": dict(COLOR_JITTER=0.4)}


def strong(args, dev):
    """--strong: DatasetMapper.map_batch (training) with train_aug on 480 x 640 images to 800 x 1067, for all four groups, the blur
    alone and the jitter alone.  Every configured group is APPLIED to every image (the RandomApply probabilities and the erasers'
    are forced to 1; grayscale keeps its 0.2): the most work the config can ask for.  Per group set:
        map_batch    host wall time to the synchronised dicts: device (resize + augmentation launches), resize_only (the same
                     mapper without train_aug), host (LOCOV_FUSED_AUGMENT=0: strong_augment.apply_host per image)
        launches     ops.augment_images on images already on the device: device-event time per call and each launch's device time
                     (torch.profiler), beside the algorithmic bytes -- every image read and written once, the contrast pass's
                     second read, the erasers' noise -- at the measured copy rate --copy-tbs
        pillow       the reference's own chain (ImageEnhance / convert / GaussianBlur, the erasers' torch expression) on the
                     resized images with the same draws, then .to(device): one thread, and a pool of --threads threads"""
    import locov_amd
    from locov_amd import data, ops
    from locov_amd import strong_augment as sa
    try:
        from PIL import Image, ImageEnhance, ImageFilter
    except ImportError:
        Image = None
    h, w = 480, 640
    rec = {"device": torch.cuda.get_device_name(dev), "source": [h, w], "copy_tbs": args.copy_tbs, "runs": {}}
    pool = ThreadPoolExecutor(max_workers=args.threads)

    def pillow_one(chw, d, noise):
        im = Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0)), "RGB")
        enhancers = {sa.OP_BRIGHTNESS: (ImageEnhance.Brightness, d["brightness"]), sa.OP_CONTRAST: (ImageEnhance.Contrast, d["contrast"]),
                     sa.OP_SATURATION: (ImageEnhance.Color, d["saturation"])}
        for op, _ in sa.jitter_chain(d):
            if op == sa.OP_HUE:
                hh, s, v = im.convert("HSV").split()
                np_h = np.array(hh, dtype=np.uint8)
                with np.errstate(over="ignore"):
                    np_h += np.uint8(sa.hue_shift(d["hue"]))
                im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
            else:
                im = enhancers[op][0](im).enhance(enhancers[op][1])
        if d["gray"]:
            l = np.asarray(im.convert("L"))
            im = Image.fromarray(np.dstack([l, l, l]), "RGB")
        if d["blur"]:
            im = im.filter(ImageFilter.GaussianBlur(radius=d["sigma"]))
        out = np.asarray(im)
        if any(e is not None for e in d["erase"]):
            t = torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1))).float().div(255)
            at = 0
            for e in d["erase"]:
                if e is not None:
                    i, j, eh, ew = e
                    t[:, i:i + eh, j:j + ew] = noise[at:at + 3 * eh * ew].view(3, eh, ew)
                    at += 3 * eh * ew
            return t.mul(255).byte()
        return torch.as_tensor(np.ascontiguousarray(out.transpose(2, 0, 1)))

    for name, keys in STRONG_GROUPS.items():
        cfg = locov_amd.config.get_cfg()
        cfg.MODEL.DEVICE = str(dev)
        plain = data.DatasetMapper(cfg, True, device=dev, seed=1)
        for k, v in keys.items():
            cfg.INPUT[k] = v
        aug = sa.build_complete_augmentation(cfg, True)
        aug.JITTER_P = aug.BLUR_P = 1.0
        for eraser in aug.erasers:
            eraser.p = 1.0
        mapper = data.DatasetMapper(cfg, True, device=dev, seed=1, train_aug=aug)
        for N in args.images:
            rng = np.random.default_rng(N)
            dicts = [{"image_raw": rng.integers(0, 256, (h, w, 3), dtype=np.uint8)} for _ in range(N)]
            sample = mapper.draw_sample(dicts)
            noise = mapper.erase_noise(sample)
            sample["erase_noise"] = noise
            base = {k: sample[k] for k in ("short_edge", "flip", "caption")}
            resized = [d["image"] for d in plain.map_batch(dicts, base)]
            counts = [sa.noise_count(s) for s in sample["strong"]]
            offsets = [int(o) for o in np.concatenate([[0], np.cumsum(counts)[:-1]])]

            def side(fused, m=mapper, s=sample):
                def step():
                    os.environ["LOCOV_FUSED_AUGMENT"] = fused
                    return m.map_batch(dicts, s)
                return step

            got = side("1")()
            for a, b in zip(got, side("0")()):
                assert torch.equal(a["image"], b["image"]), "the device path and the definition differ"
            r = {"output": list(resized[0].shape[1:]), "sigma": [round(s["sigma"], 3) for s in sample["strong"]][:8],
                 "erased_pixels": sum(counts) // 3,
                 "map_batch": {"device": wall(side("1"), args.iters, args.warmup), "resize_only": wall(lambda: plain.map_batch(dicts, base), args.iters, args.warmup),
                               "host": wall(side("0"), args.host_iters, 1)}}
            os.environ.pop("LOCOV_FUSED_AUGMENT", None)
            launch = lambda: ops.augment_images(resized, sample["strong"], noise, offsets)
            k = kernels(launch, top=3)
            pixels = sum(int(x.shape[1] * x.shape[2]) for x in resized)
            contrast = sum(int(x.shape[1] * x.shape[2]) for x, s in zip(resized, sample["strong"]) if s["jitter"])
            nbytes = 3 * (2 * pixels + contrast) + 4 * sum(counts)
            r["launches"] = dict(alternate({"call": launch}, args.iters, args.warmup)["call"], device=k, bytes=nbytes,
                                 tbs=nbytes / (k["total_us"] * 1e-6) / 1e12, bound_us=nbytes / (args.copy_tbs * 1e12) * 1e6)
            if Image is not None:
                host_images = [x.cpu().numpy() for x in resized]
                host_noise = noise.cpu()
                jobs = [(x, s, host_noise[o:o + c]) for x, s, o, c in zip(host_images, sample["strong"], offsets, counts)]
                for a, j in zip(got, jobs):
                    assert torch.equal(a["image"].cpu(), pillow_one(*j)), "the device path and Pillow differ"
                r["pillow"] = {"1_thread": wall(lambda: [pillow_one(*j).to(dev) for j in jobs], args.host_iters, 1),
                               f"{args.threads}_threads": wall(lambda: [y.to(dev) for y in pool.map(lambda j: pillow_one(*j), jobs)],
                                                               args.host_iters, 1)}
            rec["runs"][f"{name}_images_{N}"] = r
            print(json.dumps({f"strong {name} images {N}": r}), flush=True)
    return rec


def _photo_like(rng, h, w):
    """A synthetic image with a photograph's spectrum rather than white noise: low-pass noise at three scales plus a little grain."""
    out = np.zeros((h, w, 3), np.float32)
    for cell, gain in ((64, 70.0), (16, 35.0), (4, 12.0)):
        coarse = rng.standard_normal((h // cell + 2, w // cell + 2, 3)).astype(np.float32)
        t = torch.from_numpy(coarse).permute(2, 0, 1)[None]
        up = torch.nn.functional.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
        out += gain * up
    out += 128.0 + 3.0 * rng.standard_normal((h, w, 3)).astype(np.float32)
    return np.clip(out, 0, 255).astype(np.uint8)


def jpeg(args, dev):
    """--jpeg: DatasetMapper.map_batch FROM FILES, the images of the default rows (white noise, 480 x 640 and 3000 x 4000, to
    800 x 1067) and photograph-like ones of the same sizes, encoded by Pillow at quality 90, 4:2:0.  Per size and content:
        map_batch    host wall time to the synchronised dicts, the two sides alternating in one process: device (the scans on
                     host threads, one pinned upload, two launches, then the resize's one) and pillow (LOCOV_FUSED_JPEG=0: the path
                     before the decoder existed, every file through Pillow on one thread, then the upload of the raw bytes)
        pillow       Image.open(...).convert("RGB") alone, from memory: one thread, and a pool of --threads threads
        entropy      ops.jpeg_entropy_stage alone: a call per image (one thread), and one call for the batch (min(16, n) threads)
        pack / upload   ops.jpeg_pack into the pinned buffer (host wall), and its copy to the device (device-event time)
        launches     ops.jpeg_decode_records on records already on the device: device-event time per call, each launch's device time
        bytes        the record's bytes per pixel beside the file's and the raw image's 3"""
    import io
    import tempfile
    import locov_amd
    from locov_amd import data, ops
    from PIL import Image
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.DEVICE = str(dev)
    mapper = data.DatasetMapper(cfg, False, device=dev)
    rec = {"device": torch.cuda.get_device_name(dev), "quality": 90, "subsampling": "4:2:0", "threads": args.threads, "runs": {}}
    pool = ThreadPoolExecutor(max_workers=args.threads)
    N = max(args.images)
    tmp = tempfile.mkdtemp(prefix="time_data_jpeg_")
    for h, w in SOURCES:
        big = h * w > 1 << 21
        iters, warmup = (args.jpeg_big_iters, 2) if big else (args.iters, args.warmup)
        for content in ("noise", "photo"):
            rng = np.random.default_rng(N)
            raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if content == "noise" else _photo_like(rng, h, w) for _ in range(N)]
            datas, dicts = [], []
            for i, x in enumerate(raws):
                buf = io.BytesIO()
                Image.fromarray(x).save(buf, "JPEG", quality=90, subsampling="4:2:0")
                datas.append(buf.getvalue())
                path = os.path.join(tmp, f"{content}_{h}x{w}_{i}.jpg")
                with open(path, "wb") as f:
                    f.write(datas[-1])
                dicts.append({"file_name": path, "height": h, "width": w})
            del raws

            def side(fused):
                def step():
                    os.environ["LOCOV_FUSED_JPEG"] = fused
                    return mapper.map_batch(dicts)
                return step

            sides = {"device": side("1"), "pillow": side("0")}
            for a, b in zip(sides["device"](), sides["pillow"]()):
                assert torch.equal(a["image"], b["image"]), "the device path and Pillow differ"
            ms = {k: [] for k in sides}
            names = list(sides)
            for it in range(warmup + iters):
                for k in (names if it % 2 == 0 else names[::-1]):
                    t = wall(sides[k], 1, 0)
                    if it >= warmup:
                        ms[k].append(t["median_ms"])
            os.environ.pop("LOCOV_FUSED_JPEG", None)
            spread = lambda v: {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
            r = {"images": N, "source": [h, w], "iters": iters, "map_batch": {k: spread(v) for k, v in ms.items()}}
            pil = lambda d: np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))
            host_iters = max(args.host_iters, 3)
            r["pillow"] = {"1_thread": wall(lambda: [pil(d) for d in datas], host_iters, 1),
                           f"{args.threads}_threads": wall(lambda: list(pool.map(pil, datas)), host_iters, 1)}
            r["entropy"] = {"1_thread": wall(lambda: [ops.jpeg_entropy_stage([d]) for d in datas], host_iters, 1),
                            "batched": wall(lambda: ops.jpeg_entropy_stage(datas), host_iters, 1)}
            staged = ops.jpeg_entropy_stage(datas)
            assert all(s.status == 0 for s in staged)
            r["pack"] = wall(lambda: ops.jpeg_pack(staged, pin_memory=True), host_iters, 1)
            batch = ops.jpeg_pack(staged, pin_memory=True)
            r["upload"] = alternate({"copy": lambda: batch.records.to(dev, non_blocking=True)}, iters, warmup)["copy"]
            records = batch.records.to(dev)
            launch = lambda: ops.jpeg_decode_records(records, batch.descs, cfg.INPUT.FORMAT)
            r["launches"] = dict(alternate({"call": launch}, iters, warmup)["call"], device=kernels(launch, top=2))
            pixels = N * h * w
            r["bytes_per_pixel"] = {"record": batch.records.numel() / pixels, "file": sum(len(d) for d in datas) / pixels, "raw": 3.0}
            del records, batch, staged
            rec["runs"][f"{content}_{h}x{w}_images_{N}"] = r
            print(json.dumps({f"jpeg {content} {h}x{w} images {N}": r}), flush=True)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--jpeg", action="store_true", help="time the mapper from JPEG files instead (see jpeg())")
    ap.add_argument("--jpeg-big-iters", type=int, default=8, help="--jpeg: timed iterations of the two map_batch sides at 3000 x 4000 (a Pillow "
                    "side takes seconds per iteration), after two warm-ups")
    ap.add_argument("--strong", action="store_true", help="time the strong augmentation of the mapper instead (see strong())")
    ap.add_argument("--proposals", type=int, default=0, help="rows per image: time the proposal side of the mapper instead (see proposals())")
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=3, help="timed iterations of the host-path and Pillow sides (after one warm-up)")
    ap.add_argument("--threads", type=int, default=16, help="size of the Pillow thread pool")
    ap.add_argument("--copy-tbs", type=float, default=6.29, help="measured device copy rate the kernel's byte rate is put beside, TB/s")
    ap.add_argument("--out", default=None, help="also write the record as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_data: needs a ROCm GPU")
    if args.iters < 50 or args.warmup < 10:
        raise SystemExit("time_data: the protocol asks for >= 10 warm-up and >= 50 timed iterations")
    if args.proposals > 0 or args.strong or args.jpeg:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        rec = jpeg(args, dev) if args.jpeg else strong(args, dev) if args.strong else proposals(args, dev)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
        return
    import locov_amd
    from locov_amd import data, ops
    try:
        import PIL
        from PIL import Image
    except ImportError:
        PIL = Image = None
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.DEVICE = str(dev)
    on_device, on_host = data.DatasetMapper(cfg, False, device=dev), data.DatasetMapper(cfg, False, device="cpu")
    rec = {"device": torch.cuda.get_device_name(dev), "pillow": PIL.__version__ if PIL else None, "torch_threads": torch.get_num_threads(),
           "pillow_threads": [1, args.threads], "host_path_threads": 1, "runs": {}}
    pool = ThreadPoolExecutor(max_workers=args.threads)

    def pillow_one(img, size):
        return torch.as_tensor(np.ascontiguousarray(np.asarray(Image.fromarray(img).resize((size[1], size[0]), Image.BILINEAR)).transpose(2, 0, 1)))

    for h, w in SOURCES:
        size = data.ResizeShortestEdge.get_output_shape(h, w, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
        for N in args.images:
            rng = np.random.default_rng(N)
            raws = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(N)]
            dicts = [{"image_raw": x} for x in raws]
            on_gpu = [torch.from_numpy(x).to(dev) for x in raws]
            r = {"source": [h, w], "output": list(size), "supported": ops.resize_supported((h, w), size, 3)}
            # (a)
            step = lambda: ops.resize_flip_images(on_gpu, [size] * N)
            t = alternate({"kernel": step}, args.iters, args.warmup)["kernel"]
            k = kernels(step, top=2)
            nbytes = N * 3 * (h * w + size[0] * size[1])
            r["kernel"] = dict(t, device=k, bytes=nbytes, tbs=nbytes / (k["total_us"] * 1e-6) / 1e12, copy_tbs=args.copy_tbs,
                               bound_us=nbytes / (args.copy_tbs * 1e12) * 1e6)
            # (b)
            got = on_device.map_batch(dicts)
            sides = {"device": (lambda: on_device.map_batch(dicts), args.iters, args.warmup),
                     "host": (lambda: [d["image"].to(dev) for d in on_host.map_batch(dicts)], args.host_iters, 1)}
            if Image is not None:
                sides["pillow_1_thread"] = (lambda: [pillow_one(x, size).to(dev) for x in raws], args.host_iters, 1)
                sides[f"pillow_{args.threads}_threads"] = (lambda: [y.to(dev) for y in pool.map(lambda x: pillow_one(x, size), raws)],
                                                           args.host_iters, 1)
                for a, b in zip(got, sides["pillow_1_thread"][0]()):
                    assert torch.equal(a["image"], b), "the device path and Pillow differ"
            r["map_batch"] = {name: wall(s, iters, warmup) for name, (s, iters, warmup) in sides.items()}
            rec["runs"][f"{h}x{w}_images_{N}"] = r
            print(json.dumps({f"{h}x{w} images {N}": r}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
