"""Writes tests/golden/g14_jpeg.npz: small JPEG streams written by the installed Pillow, and Pillow's own decode of each
(np.asarray(Image.open(...).convert("RGB"))), what locov_amd.jpeg.decode_jpeg_host must reproduce byte for byte.

Run by hand where Pillow is installed (python tests/golden/make_golden_g14.py); the tests read the file and need no Pillow.  Every
image is synthetic (a seeded generator), nothing is read from outside.  The file holds

  names            one per stream ("<kind>_<w>x<h>_<layout>_q<quality>[_<extra>]")
  kind             "ok" (a stream the device decoder takes), "scaled" (quantisers multiplied: the decoder refuses it or gives Pillow's
                   bytes) or the reason it must fall back: "progressive", "cut", "no_eoi", "sampling", "png"
  data, data_off   the streams' bytes back to back and their offsets (len(names) + 1)
  rgb, rgb_off     Pillow's RGB bytes of the "ok" and "scaled" streams back to back (nothing for the others), and their offsets
  width, height    per stream (0 for the PNG)
  pillow_version, libjpeg_turbo_version
"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 23), (33, 9), (2, 35), (40, 24)]                # (width, height)
TINY = [(3, 3), (4, 4), (35, 2), (5, 3), (6, 17)]                                                # around jdsample.c's `downsampled_width > 2`
LAYOUTS = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0", "grey": None}


def smooth(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 127.5 + 127.5 * np.sin(0.21 * x + 0.13 * y)
    g = 255.0 * (x + 2 * y) / max(w + 2 * h - 3, 1)
    b = 127.5 + 127.5 * np.cos(0.17 * x - 0.29 * y + 1.0)
    return np.clip(np.stack([r, g, b], axis=-1) + 0.5, 0, 255).astype(np.uint8)


def noise(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def black_white(rng, w, h):
    return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def encode(img, layout, quality, **kw):
    from PIL import Image
    im = Image.fromarray(img)
    if layout == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = LAYOUTS[layout]
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def with_segments(data):
    """A COM segment and an APP5 segment behind the stream's first segment, fill bytes in front of the second."""
    assert data[:2] == b"\xff\xd8" and data[2] == 0xFF
    first = 4 + ((data[4] << 8) | data[5])
    com = b"\xff\xfe" + (2 + 11).to_bytes(2, "big") + b"hello there"
    app = b"\xff\xff\xff\xe5" + (2 + 6).to_bytes(2, "big") + b"\0\1\2\3\xff\xd9"
    return data[:first] + com + app + data[first:]


def as_440(data):
    """A 4:2:2 stream whose frame header claims 2 x 1 luma blocks stacked instead of side by side: the 4:4:0 layout, for the header."""
    at = data.index(b"\xff\xc0")
    assert data[at + 11] == 0x21
    return data[:at + 11] + b"\x12" + data[at + 12:]


def scale_dqt(data, factor):
    """The stream with every 8-bit quantiser multiplied by `factor` (at most 255)."""
    out = bytearray(data)
    at = 2
    while out[at + 1] != 0xDA:
        seg = (out[at + 2] << 8) | out[at + 3]
        if out[at + 1] == 0xDB:
            p = at + 4
            while p < at + 2 + seg:
                assert out[p] >> 4 == 0
                out[p + 1:p + 65] = bytes(min(255, q * factor) for q in out[p + 1:p + 65])
                p += 65
        at += 2 + seg
    return bytes(out)


def main():
    import PIL
    from PIL import Image, features
    rng = np.random.default_rng(1414)
    streams = []                                                  # (name, kind, bytes)

    def add(name, data, kind="ok"):
        assert name not in [s[0] for s in streams], name
        streams.append((name, kind, data))

    for w, h in SIZES:
        for layout in LAYOUTS:
            add(f"smooth_{w}x{h}_{layout}_q75", encode(smooth(w, h), layout, 75))
    for w, h in TINY:
        for layout in ("422", "420"):
            add(f"noise_{w}x{h}_{layout}_q90", encode(noise(rng, w, h), layout, 90))
    for q in (1, 30, 75, 95, 100):
        add(f"smooth_17x23_420_q{q}_b", encode(smooth(17, 23), "420", q))
        add(f"noise_17x23_420_q{q}", encode(noise(rng, 17, 23), "420", q))
    add("noise_9x9_444_q100", encode(noise(rng, 9, 9), "444", 100))
    add("bw_16x33_420_q90", encode(black_white(rng, 16, 33), "420", 90))
    add("bw_16x33_grey_q50", encode(black_white(rng, 16, 33), "grey", 50))
    add("noise_16x16_420_q75_optimize", encode(noise(rng, 16, 16), "420", 75, optimize=True))
    add("smooth_33x9_422_q5_optimize", encode(smooth(33, 9), "422", 5, optimize=True))
    add("noise_40x24_420_q75_rst2", encode(noise(rng, 40, 24), "420", 75, restart_marker_blocks=2))
    add("smooth_40x24_444_q75_rst2", encode(smooth(40, 24), "444", 75, restart_marker_blocks=2))
    add("noise_40x24_422_q75_rstrow", encode(noise(rng, 40, 24), "422", 75, restart_marker_rows=1))
    add("noise_40x24_grey_q75_rst2", encode(noise(rng, 40, 24), "grey", 75, restart_marker_blocks=2))
    add("smooth_17x23_420_q75_segments", with_segments(encode(smooth(17, 23), "420", 75)))
    mixed = smooth(70, 150)
    mixed[40:110, 20:60] = noise(rng, 40, 70)
    add("mixed_70x150_420_q90", encode(mixed, "420", 90))
    # what must fall back
    add("smooth_17x23_420_q75_progressive", encode(smooth(17, 23), "420", 75, progressive=True), "progressive")
    whole = encode(noise(rng, 40, 24), "420", 75)
    add("noise_40x24_420_q75_cut", whole[:len(whole) // 2], "cut")
    add("noise_40x24_420_q75_cut_scan", whole[:len(whole) - 40], "cut")
    assert whole[-2:] == b"\xff\xd9"
    add("noise_40x24_420_q75_noeoi", whole[:-2], "no_eoi")
    add("smooth_16x16_440_q75", as_440(encode(smooth(16, 16), "422", 75)), "sampling")
    buf = io.BytesIO()
    Image.fromarray(smooth(9, 7)).save(buf, "PNG")
    add("smooth_9x7_png", buf.getvalue(), "png")

    # quality-100 streams with their quantisers scaled up: reconstructions far outside [0, 255], where libjpeg's wrapping range-limit
    # table and libjpeg-turbo's saturating SIMD code part ways.  Each must be refused by the decoder or decoded to Pillow's bytes.
    rng2 = np.random.default_rng(2828)
    for content, make in (("noise", noise), ("bw", black_white)):
        for w, h in ((8, 8), (16, 16), (17, 23)):
            for layout in ("444", "422", "420"):
                base = encode(make(rng2, w, h), layout, 100)
                for factor in (3, 4, 6):
                    add(f"{content}_{w}x{h}_{layout}_q100_dqt{factor}", scale_dqt(base, factor), "scaled")

    rgb, width, height = [], [], []
    for name, kind, data in streams:
        if kind in ("ok", "scaled"):
            im = Image.open(io.BytesIO(data))
            px = np.asarray(im.convert("RGB"))
            assert f"_{px.shape[1]}x{px.shape[0]}_" in name, (name, px.shape)
            assert (im.mode == "L") == ("_grey_" in name), (name, im.mode)
        else:
            px = np.zeros((0, 0, 3), np.uint8)
        rgb.append(px.reshape(-1))
        width.append(px.shape[1])
        height.append(px.shape[0])
    out = {
        "names": np.array([s[0] for s in streams]), "kind": np.array([s[1] for s in streams]),
        "data": np.frombuffer(b"".join(s[2] for s in streams), np.uint8),
        "data_off": np.cumsum([0] + [len(s[2]) for s in streams]).astype(np.int64),
        "rgb": np.concatenate(rgb), "rgb_off": np.cumsum([0] + [len(r) for r in rgb]).astype(np.int64),
        "width": np.array(width, np.int32), "height": np.array(height, np.int32),
        "pillow_version": np.array(PIL.__version__), "libjpeg_turbo_version": np.array(str(features.version("libjpeg_turbo"))),
    }
    path = os.path.join(HERE, "g14_jpeg.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(streams)} streams, {sum(len(s[2]) for s in streams)} stream bytes, "
          f"Pillow {PIL.__version__}, libjpeg-turbo {features.version('libjpeg_turbo')}")


if __name__ == "__main__":
    main()
