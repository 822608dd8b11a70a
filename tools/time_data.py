"""The input pipeline (locov_amd/data.py): DatasetMapper.map_batch on the device against its own host path and, where Pillow imports,
against Pillow on the same machine; and the resize kernel alone.

    timeout -k 10 600 python tools/time_data.py [--images 1 8] [--iters 50] [--warmup 10] [--threads 16] [--out records.json]

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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
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
