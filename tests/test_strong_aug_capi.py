"""locov_augment_images / locov_augment_supported / locov_augment_images_workspace_bytes on the CPU: argument errors are returned
before any HIP call (there is no GPU here), and the supported sigma range holds the reference's [0.1, 2.0]."""
import ctypes

import numpy as np
import pytest

import strong_aug_ref as ref


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def _desc(_lib, n=1, h=8, w=9):
    descs = (_lib.AugmentDesc * n)()
    for d in descs:
        d.height, d.width, d.brightness, d.contrast, d.saturation = h, w, 1.0, 1.0, 1.0
    return descs


def _call(lib, descs, n, images=None, outs=None, noise=ctypes.c_void_p(4096), n_noise=0, workspace=ctypes.c_void_p(1 << 20), ws_bytes=1 << 20):
    images = (ctypes.c_void_p * max(n, 1))(*[256 + 64 * i for i in range(max(n, 1))]) if images is None else images
    outs = (ctypes.c_void_p * max(n, 1))(*[65536 + 64 * i for i in range(max(n, 1))]) if outs is None else outs
    return lib.locov_augment_images(images, outs, descs, n, noise, n_noise, workspace, ws_bytes, None)


def test_the_supported_sigma_range(lib):
    from locov_amd import strong_augment as sa
    for sigma in np.linspace(0.1, 2.0, 200):
        assert lib.locov_augment_supported(float(sigma)) == 1
    assert lib.locov_augment_supported(2.4) == 1 and lib.locov_augment_supported(2.5) == 0        # the box radius reaches 2 at sqrt(6)
    for sigma in (0.0, -1.0, 40.0, float("nan"), float("inf")):
        assert lib.locov_augment_supported(sigma) == 0
    for sigma in (0.1, 1.0, 2.0, 2.4, 2.5, 3.0):                                                  # the library's rule is the definition's reach
        assert lib.locov_augment_supported(sigma) == int(sa.blur_reach(sigma) <= 2) == int(int(ref.box_radius(sigma)) + 1 <= 2)


def test_argument_errors_come_before_any_hip_call(lib):
    from locov_amd import _lib
    err = lambda: lib.locov_last_error()
    assert lib.locov_augment_images(None, None, None, 0, None, 0, None, 0, None) == 0            # no images: a no-op
    descs = _desc(_lib)
    assert lib.locov_augment_images(None, None, descs, 1, None, 0, ctypes.c_void_p(1 << 20), 1 << 20, None) == -1 and b"null pointer" in err()
    assert _call(lib, None, 1) == -1 and b"null pointer" in err()
    assert _call(lib, descs, 1, workspace=None) == -1 and b"null pointer" in err()
    assert _call(lib, descs, 1, images=(ctypes.c_void_p * 1)(None)) == -1 and b"null pointer (image 0)" in err()
    assert _call(lib, descs, 1, images=(ctypes.c_void_p * 1)(512), outs=(ctypes.c_void_p * 1)(512)) == -1 and b"must not be the input" in err()
    many = _desc(_lib, _lib.LABEL_MAX_IMAGES + 1)
    assert _call(lib, many, _lib.LABEL_MAX_IMAGES + 1) == -1 and b"images per call" in err()
    assert _call(lib, descs, -1) == -1
    for h, w in ((0, 9), (8, 0), (-3, 4)):
        assert _call(lib, _desc(_lib, 1, h, w), 1) == -1 and b"sizes must be positive" in err()
    assert _call(lib, _desc(_lib, 1, 40000, 40000), 1) == -1 and b"int32" in err()

    d = _desc(_lib)
    d[0].n_ops, d[0].ops[0] = 1, 5
    assert _call(lib, d, 1) == -1 and b"unknown operation 5" in err()
    d[0].ops[0] = 0
    assert _call(lib, d, 1) == -1 and b"unknown operation 0" in err()
    d[0].n_ops, d[0].ops[0], d[0].ops[1], d[0].ops[2] = 3, 2, 4, 2
    assert _call(lib, d, 1) == -1 and b"repeated operation 2" in err()
    d[0].n_ops = 5
    assert _call(lib, d, 1) == -1 and b"jitter operations" in err()

    d = _desc(_lib)
    for sigma in (2.5, -0.5, float("nan")):
        d[0].sigma = sigma
        assert _call(lib, d, 1) == -1 and b"sigma" in err()
    d = _desc(_lib)
    d[0].hue_shift = 256
    assert _call(lib, d, 1) == -1 and b"hue_shift" in err()
    d = _desc(_lib)
    d[0].contrast = float("inf")
    assert _call(lib, d, 1) == -1 and b"not finite" in err()

    d = _desc(_lib)                                                                               # 8 x 9
    d[0].n_erase = 4
    assert _call(lib, d, 1) == -1 and b"erasers" in err()
    d[0].n_erase = 1
    d[0].erase[0][:] = [3, 0, 6, 2]                                                               # rows 3 .. 8 of 8
    assert _call(lib, d, 1, n_noise=1000) == -1 and b"leaves the image" in err()
    d[0].erase[0][:] = [3, 0, 5, 2]                                                               # 30 values
    d[0].noise_offset = 971
    assert _call(lib, d, 1, n_noise=1000) == -1 and b"past the tensor" in err()
    d[0].noise_offset = -1
    assert _call(lib, d, 1, n_noise=1000) == -1 and b"negative noise offset" in err()
    d[0].noise_offset = 0
    assert _call(lib, d, 1, noise=None, n_noise=1000) == -1 and b"null noise" in err()
    d[0].n_erase, d[0].erase[1][:] = 2, [0, 0, 7, 8]                                              # the second block starts behind the first
    assert _call(lib, d, 1, n_noise=30 + 167) == -1 and b"eraser 1" in err()

    d = _desc(_lib)
    assert _call(lib, d, 1, workspace=ctypes.c_void_p((1 << 20) + 4)) == -1 and b"misaligned" in err()
    assert _call(lib, d, 1, ws_bytes=16) == -1 and b"workspace of 16 bytes" in err()


def test_the_workspace_holds_the_table_and_the_contrast_partials(lib):
    from locov_amd import _lib
    d = _desc(_lib, 3, 100, 130)                                                                  # 13 000 pixels: four partials of 4 096
    base = lib.locov_augment_images_workspace_bytes(d, 3)
    assert base > 0 and base % 256 == 0
    d[1].n_ops, d[1].ops[0], d[1].ops[1] = 2, 1, 2
    assert lib.locov_augment_images_workspace_bytes(d, 3) == base + 4 * 4
    d[2].n_ops, d[2].ops[0] = 1, 2
    assert lib.locov_augment_images_workspace_bytes(d, 3) == base + 8 * 4
    assert lib.locov_augment_images_workspace_bytes(d, 0) == 0 and lib.locov_augment_images_workspace_bytes(None, 3) == 0
    assert _call(lib, d, 3, ws_bytes=base + 8 * 4 - 1) == -1 and b"needed" in lib.locov_last_error()


def test_the_wrapper_refuses_cpu_tensors():
    import torch
    from locov_amd import ops
    from locov_amd._lib import LocovError
    import strong_aug_cases as sc
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.augment_images([torch.zeros(3, 4, 5, dtype=torch.uint8)], [sc.draws()])
    assert ops.augment_images([], []) == []
    assert ops.augment_supported(2.0) and not ops.augment_supported(2.5) and not ops.augment_supported(float("nan"))
