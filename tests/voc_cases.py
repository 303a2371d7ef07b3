"""Helper (not a test): writes a tiny VOCdevkit with Pillow -- JPEGs of distinct sizes, annotation XMLs and the
``ImageSets/Main`` lists -- so the VOC reader and the batched ingest run on real files.  Nothing binary is committed: the
files are written at test time.  The expected values below come from the chosen integers, not from the reader."""
import os

import numpy as np

CLASSES = sorted(["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
                  "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"])

# id, H, W, mode, objects: (class, xmin, ymin, xmax, ymax, difficult, truncated); difficult None = no <difficult> tag
IMAGES_2007 = [
    ("000001", 375, 500, "RGB", [("dog", 48, 240, 195, 371, 0, 1), ("person", 8, 12, 352, 370, 0, 0),
                                 ("chair", 263, 211, 324, 339, 1, 0)]),
    ("000002", 500, 375, "RGB", [("train", 139, 200, 207, 301, 0, 0)]),
    ("000003", 333, 500, "L", [("sofa", 123, 155, 215, 195, 1, 0), ("chair", 239, 156, 307, 205, 0, 1)]),
    ("000004", 1, 37, "RGB", [("car", 3, 0, 30, 1, 0, 0)]),
    ("000005", 120, 87, "RGB", [("cat", 1, 1, 87, 120, None, 0), ("tvmonitor", 10, 20, 40, 60, None, 0)]),
    ("000006", 41, 1, "RGB", [("bottle", 0, 5, 1, 33, 1, 0)]),
    ("000007", 300, 300, "RGB", [("horse", 69, 172, 270, 300, 0, 0), ("person", 150, 141, 229, 284, 0, 0),
                                 ("person", 285, 201, 300, 250, 1, 1), ("aeroplane", 5, 5, 100, 50, 0, 0)]),
    ("000008", 281, 300, "RGB", [("bicycle", 54, 50, 285, 262, 0, 0)]),
    ("000009", 299, 301, "RGB", [("bird", 90, 125, 237, 212, 1, 0)]),
    ("000010", 442, 500, "RGB", [("pottedplant", 20, 30, 140, 430, 0, 0), ("diningtable", 100, 200, 499, 441, 1, 1),
                                 ("cow", 1, 1, 2, 2, 0, 0)]),
]
SPLITS_2007 = {"train": ["000001", "000005", "000007", "000008"], "val": ["000002", "000003", "000009"],
               "test": ["000010", "000004", "000006"]}
IMAGES_2012 = [
    ("2008_000008", 442, 500, "RGB", [("horse", 53, 87, 471, 420, 0, 0), ("person", 158, 44, 289, 167, 0, 1)]),
    ("2008_000015", 500, 333, "RGB", [("bottle", 270, 1, 378, 176, 0, 0)]),
    ("2008_000019", 360, 480, "RGB", [("dog", 139, 2, 372, 197, None, 0)]),
]
SPLITS_2012 = {"train": ["2008_000008", "2008_000019"], "val": ["2008_000015"]}          # no test.txt, as in VOC2012 trainval


def pixels(h, w, mode, seed):
    """Smooth content plus a little noise (so JPEG keeps some structure): uint8 [h,w,3] or [h,w] for mode L."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(1 if mode == "L" else 3):
        f = 127.5 + 90.0 * np.sin(yy / (7.0 + 3 * c) + seed) * np.cos(xx / (11.0 - 2 * c)) + rng.normal(0, 12.0, (h, w))
        chans.append(np.clip(f, 0, 255).astype(np.uint8))
    return chans[0] if mode == "L" else np.stack(chans, -1)


def xml_text(image_id, h, w, mode, objects, class_name=None):
    parts = ["<annotation>", "<folder>VOC</folder>", "<filename>%s.jpg</filename>" % image_id,
             "<size><width>%d</width><height>%d</height><depth>%d</depth></size>" % (w, h, 1 if mode == "L" else 3),
             "<segmented>0</segmented>"]
    for name, xmin, ymin, xmax, ymax, difficult, truncated in objects:
        parts.append("<object><name>%s</name><pose>Unspecified</pose><truncated>%d</truncated>" % (class_name or name, truncated))
        if difficult is not None:
            parts.append("<difficult>%d</difficult>" % difficult)
        parts.append("<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>" % (
            xmin, ymin, xmax, ymax))
    parts.append("</annotation>")
    return "\n".join(parts) + "\n"


def write_year(root, year, images, splits):
    """``<root>/VOCdevkit/VOC<year>``; returns ``{id: the array that was encoded}``."""
    from PIL import Image
    base = os.path.join(str(root), "VOCdevkit", "VOC" + year)
    for sub in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    encoded = {}
    for n, (image_id, h, w, mode, objects) in enumerate(images):
        a = pixels(h, w, mode, seed=n + int(year))
        Image.fromarray(a, mode=mode).save(os.path.join(base, "JPEGImages", image_id + ".jpg"), quality=92)
        with open(os.path.join(base, "Annotations", image_id + ".xml"), "w") as f:
            f.write(xml_text(image_id, h, w, mode, objects))
        encoded[image_id] = a
    for name, ids in splits.items():
        with open(os.path.join(base, "ImageSets", "Main", name + ".txt"), "w") as f:
            f.write("".join(i + "\n" for i in ids))
    return encoded


def write_devkit(root, with_2012=False):
    """The 2007 devkit (and the 2012 one) under ``root``; returns ``{id: encoded array}`` of everything written."""
    encoded = write_year(root, "2007", IMAGES_2007, SPLITS_2007)
    if with_2012:
        encoded.update(write_year(root, "2012", IMAGES_2012, SPLITS_2012))
    return encoded


def spec(image_id):
    return next(s for s in IMAGES_2007 + IMAGES_2012 if s[0] == image_id)


def expected_objects(image_id):
    """What the reader must return for ``image_id``, from the integers above: float64 division, then float32."""
    _, h, w, _, objects = spec(image_id)
    bbox = np.array([[np.float64(ymin) / h, np.float64(xmin) / w, np.float64(ymax) / h, np.float64(xmax) / w]
                     for _, xmin, ymin, xmax, ymax, _, _ in objects], np.float64).reshape(-1, 4).astype(np.float32)
    return {"bbox": bbox, "label": np.array([CLASSES.index(o[0]) for o in objects], np.int64),
            "is_difficult": np.array([bool(o[5]) for o in objects], bool),
            "is_truncated": np.array([bool(o[6]) for o in objects], bool)}


def decoded(root, year, image_id):
    """Pillow's own decode of the written file."""
    from PIL import Image
    path = os.path.join(str(root), "VOCdevkit", "VOC" + year, "JPEGImages", image_id + ".jpg")
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def all_decoded_2007(root):
    return [decoded(root, "2007", s[0]) for s in IMAGES_2007]
