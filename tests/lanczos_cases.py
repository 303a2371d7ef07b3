"""Shared by the LANCZOS resize tests (tests/test_lanczos_cpu.py, tests/test_lanczos_gpu.py), the fixture script
(tests/golden/make_lanczos_golden.py) and tests/bench_resize.py: seeded source images, Pillow's 8-bit two-pass
resampler as NumPy integer arithmetic on ``data_utils.lanczos_coefficients`` tables, and live Pillow when it imports."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lanczos.npz")

# the fixture: (name, source (H, W), content); every source is resized to every FIXTURE_OUT (h, w)
FIXTURE_SOURCES = [("a", (48, 64), "noise"), ("b", (64, 48), "edges"), ("c", (20, 24), "gradient"),
                   ("d", (7, 5), "noise"), ("e", (1, 40), "noise"), ("f", (33, 16), "gradient")]
FIXTURE_OUT = [(20, 20), (24, 16), (48, 64), (64, 48)]
# the issue's size lists, (H, W): CPU test against live Pillow (-> 300 x 300) and the GPU test's ragged batch
CPU_LIVE_SIZES = [(5, 7), (7, 5), (300, 300), (300, 281), (301, 299), (1920, 1080), (87, 120), (120, 87), (375, 500),
                  (3000, 2000)]
GPU_SIZES = [(375, 500), (500, 333), (300, 300), (281, 300), (299, 301), (120, 87), (7, 5), (1, 40), (1080, 1920),
             (2000, 3000)]
GPU_OUT = [(300, 300), (512, 512), (300, 512)]
CONTENTS = ("noise", "gradient", "edges")


def image(h, w, content, seed=0):
    """Seeded uint8 [h,w,3]: uniform noise, a two-axis gradient with per-channel slopes, or binary edges (0 / 255
    blocks a few pixels wide: the content that overshoots and exercises the clamp)."""
    rng = np.random.default_rng([seed, h, w, CONTENTS.index(content)])
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if content == "gradient":
        c = np.arange(3)[None, None, :]
        return ((y[..., None] * (3 + c) + x[..., None] * (5 - c) + 17 * c) % 256).astype(np.uint8)
    by, bx = int(rng.integers(2, 6)), int(rng.integers(2, 6))
    cells = rng.integers(0, 2, (h // by + 1, w // bx + 1, 3), dtype=np.uint8) * 255
    return np.ascontiguousarray(cells[y // by, x // bx])


def _resample_axis(img, out_size, axis, coefficients):
    n = img.shape[axis]
    if n == out_size:                                   # Pillow skips the pass
        return img
    bounds, k = coefficients(n, out_size)
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + a.shape[1:], np.uint8)
    for i in range(out_size):
        xmin, xmax = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << 21) + np.tensordot(k[i, :xmax].astype(np.int64), a[xmin:xmin + xmax], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31              # Pillow's (and the kernel's) int32 accumulator does not wrap
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def two_pass(img, out_h, out_w, coefficients=None):
    """Pillow's order: horizontal pass, uint8 intermediate, vertical pass; integer arithmetic only."""
    if coefficients is None:
        from utils import data_utils
        coefficients = data_utils.lanczos_coefficients
    return np.ascontiguousarray(_resample_axis(_resample_axis(img, out_w, 1, coefficients), out_h, 0, coefficients))


def pillow_available():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


def pillow(img, out_h, out_w):
    from PIL import Image
    return np.array(Image.fromarray(img).resize((out_w, out_h), Image.LANCZOS), dtype=np.uint8)


def load_fixture():
    """{(name, out_h, out_w): (source, Pillow's output)} and the Pillow version that wrote it."""
    z = np.load(GOLDEN)
    cases = {}
    for name, _, _ in FIXTURE_SOURCES:
        for oh, ow in FIXTURE_OUT:
            cases[(name, oh, ow)] = (z["src_" + name], z["out_%s_%dx%d" % (name, oh, ow)])
    return cases, str(z["pillow_version"])
