"""PASCAL VOC 2007 / 2012 from a VOCdevkit directory on disk: what ``tfds.load("voc/2007", ...)`` hands the reference
(utils/data_utils.py:32-45), without tensorflow_datasets and without downloading anything.

[3P, unpinned: TF / tfds cannot be imported here -- DESIGN.md section 3] The annotation semantics restate the tfds VOC
builder: objects in XML order; ``bbox = float32(ymin / height, xmin / width, ymax / height, xmax / width)`` divided in
float64 by the XML's own ``<size>``, no -1 offset; ``label`` = index into the alphabetical class list; ``is_difficult =
bool(int(difficult))``, False when the tag is absent (``is_truncated`` likewise).

Annotations are parsed with ``xml.etree`` (on first use, cached); images are decoded only when an item is asked for, by
``PIL.Image.open(...).convert("RGB")`` -- the call ``data_utils._decode_custom_image`` makes."""
import os
import xml.etree.ElementTree as ET

import numpy as np

VOC_LABELS = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
              "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa",
              "train", "tvmonitor"]
SPLITS = ["train", "train+validation", "validation", "test"]
_SPLIT_FILES = {"train": ["train.txt"], "validation": ["val.txt"], "test": ["test.txt"],
                "train+validation": ["train.txt", "val.txt"]}
_NAMES = {"voc/2007": "2007", "voc/2012": "2012"}
_UNAVAILABLE = ("tensorflow_datasets is not available; use synthetic_dataset() or feed arrays "
                "[B,S,S,3] float32 in [0,1] directly")


class _Split(object):
    def __init__(self, num_examples):
        self.num_examples = num_examples


class _ClassLabel(object):
    def __init__(self, names):
        self.names = list(names)
        self.num_classes = len(self.names)


class VocInfo(object):
    """The two things the reference reads from a tfds info object: ``splits[name].num_examples`` (``train``,
    ``validation``, ``test``: the list files that exist) and ``features["labels"].names``."""

    def __init__(self, name, root, counts):
        self.name, self.root = name, root
        self.splits = {k: _Split(v) for k, v in counts.items()}
        self.features = {"labels": _ClassLabel(VOC_LABELS)}


def find_year_dir(data_dir, year):
    """``<data_dir>/VOCdevkit/VOC<year>``, where ``data_dir`` may also be the ``VOCdevkit`` or the ``VOC<year>`` folder
    itself (``~`` expanded).  Returns ``(path or None, every path looked for)``."""
    base = os.path.expanduser(str(data_dir))
    tries = [os.path.join(base, "VOCdevkit", "VOC" + year), os.path.join(base, "VOC" + year)]
    if os.path.basename(os.path.normpath(base)) == "VOC" + year:
        tries.append(base)
    for t in tries:
        if os.path.isdir(os.path.join(t, "Annotations")) and os.path.isdir(os.path.join(t, "JPEGImages")):
            return t, tries
    return None, tries


def has_year(data_dir, name):
    return find_year_dir(data_dir, _NAMES[name])[0] is not None


def _read_ids(path):
    with open(path) as f:
        return [line.split()[0] for line in f if line.strip()]


def parse_annotation(xml_path):
    """One ``Annotations/<id>.xml`` -> ``{"filename", "height", "width", "bbox" float32 [G,4], "label" int64 [G],
    "is_difficult" bool [G], "is_truncated" bool [G]}``."""
    root = ET.parse(xml_path).getroot()
    size = root.find("size")
    height, width = float(size.find("height").text), float(size.find("width").text)
    boxes, labels, difficult, truncated = [], [], [], []

    def flag(obj, tag):
        node = obj.find(tag)
        return bool(int(node.text)) if node is not None and node.text and node.text.strip() else False
    for obj in root.findall("object"):
        name = obj.find("name").text.strip()
        if name not in VOC_LABELS:
            raise ValueError("%s: class %r is not one of the 20 VOC classes" % (xml_path, name))
        bb = obj.find("bndbox")
        xmin, ymin, xmax, ymax = (float(bb.find(t).text) for t in ("xmin", "ymin", "xmax", "ymax"))
        boxes.append([ymin / height, xmin / width, ymax / height, xmax / width])      # float64 division, then float32
        labels.append(VOC_LABELS.index(name))
        difficult.append(flag(obj, "difficult"))
        truncated.append(flag(obj, "truncated"))
    fn = root.find("filename")
    return {"filename": fn.text.strip() if fn is not None and fn.text else os.path.basename(xml_path)[:-4] + ".jpg",
            "height": int(height), "width": int(width),
            "bbox": np.asarray(boxes, np.float64).reshape(-1, 4).astype(np.float32),
            "label": np.asarray(labels, np.int64), "is_difficult": np.asarray(difficult, bool),
            "is_truncated": np.asarray(truncated, bool)}


class VocDataset(object):
    """A lazy sequence of VOC items.  ``entries``: ``(year directory, image id)`` pairs in split order."""

    def __init__(self, entries, shuffle=None, records=None):
        self._entries = list(entries)
        self._records = records          # parsed annotations of ``entries`` once they were asked for
        self._shuffle = shuffle          # None or (buffer_size, seed)
        self._passes = 0

    def _subset(self, pick):
        """The entries ``pick`` selects, with the parsed records that go with them and the same shuffle."""
        return VocDataset(self._entries[pick], self._shuffle, None if self._records is None else self._records[pick])

    def __len__(self):
        return len(self._entries)

    @property
    def records(self):
        """The parsed annotations in split order (no image is decoded); each also carries ``image_path``."""
        if self._records is None:
            recs = []
            for root, image_id in self._entries:
                r = parse_annotation(os.path.join(root, "Annotations", image_id + ".xml"))
                path = os.path.join(root, "JPEGImages", r["filename"])
                if not os.path.exists(path):
                    path = os.path.join(root, "JPEGImages", image_id + ".jpg")
                r["image_path"] = path
                recs.append(r)
            self._records = recs
        return self._records

    def concatenate(self, other):
        """``Dataset.concatenate``: this dataset's items, then ``other``'s (trainer.py's ``with_voc_2012``)."""
        if self._shuffle is not None or other._shuffle is not None:
            raise ValueError("concatenate the datasets first, then shuffle the result (a shuffled operand's order would be lost)")
        both = None if self._records is None or other._records is None else self._records + other._records
        return VocDataset(self._entries + other._entries, records=both)

    def take(self, count):
        """The first ``count`` items of the split order (``Dataset.take`` before any ``shuffle``); a shuffle stays set."""
        return self._subset(slice(0, max(int(count), 0)))

    def shard(self, num_shards, index):
        """``Dataset.shard`` on the split order: every ``num_shards``-th item, starting at ``index`` (one shard per
        training rank); a shuffle stays set."""
        if not 0 <= int(index) < int(num_shards):
            raise ValueError("shard index %r outside 0..%r" % (index, int(num_shards) - 1))
        return self._subset(slice(int(index), None, int(num_shards)))

    def shuffle(self, buffer_size, seed=None):
        """``Dataset.shuffle(buffer_size, seed)``: a buffer shuffle -- the buffer holds the next ``buffer_size`` items,
        each step yields a uniformly drawn one and refills its slot.  Seeded: a fresh ``shuffle(n, seed)`` object
        always starts with the same order; every further pass over the same object draws a new one
        (``reshuffle_each_iteration``)."""
        return VocDataset(self._entries, (max(int(buffer_size), 1), 0 if seed is None else int(seed)), self._records)

    def order(self):
        """Indices into ``records`` for one pass."""
        n = len(self._entries)
        if self._shuffle is None:
            return list(range(n))
        size, seed = self._shuffle
        rng = np.random.default_rng([seed, self._passes])
        self._passes += 1
        buf, out, nxt = list(range(min(size, n))), [], min(size, n)
        while buf:
            j = int(rng.integers(len(buf)))
            out.append(buf[j])
            if nxt < n:
                buf[j] = nxt
                nxt += 1
            else:
                buf[j] = buf[-1]
                buf.pop()
        return out

    def iter_records(self):
        recs = self.records
        return [recs[i] for i in self.order()]

    @staticmethod
    def load(record):
        """Decode one record's image: the tfds-shaped dict ``data_utils.preprocessing`` consumes."""
        from PIL import Image
        image = np.asarray(Image.open(record["image_path"]).convert("RGB"), dtype=np.uint8)
        return {"image": image, "image/filename": record["filename"],
                "objects": {"bbox": record["bbox"], "label": record["label"], "is_difficult": record["is_difficult"],
                            "is_truncated": record["is_truncated"]}}

    @staticmethod
    def load_encoded(record):
        """``load`` without the decode: ``"image_bytes"`` (the file as it is on disk) takes the place of ``"image"`` when
        the file is a JPEG stream; any other file is decoded here as ``load`` does.  ``data_utils.voc_batches`` hands the
        bytes to the GPU decoder (unless ``SSD_JPEG_GPU=0``)."""
        with open(record["image_path"], "rb") as f:
            blob = f.read()
        if blob[:2] != b"\xff\xd8":
            return VocDataset.load(record)
        return {"image_bytes": blob, "image/filename": record["filename"],
                "objects": {"bbox": record["bbox"], "label": record["label"], "is_difficult": record["is_difficult"],
                            "is_truncated": record["is_truncated"]}}

    def __iter__(self):
        for r in self.iter_records():
            yield self.load(r)


def get_dataset(name, split, data_dir="~/tensorflow_datasets"):
    """``(dataset, info)`` for ``voc/2007`` / ``voc/2012`` from the devkit under ``data_dir``; ``RuntimeError`` (today's
    message plus the path looked for) when the directory or a list file of the split is not there."""
    assert split in SPLITS
    if name not in _NAMES:
        raise RuntimeError("%s (dataset %r: only voc/2007 and voc/2012 are read from disk)" % (_UNAVAILABLE, name))
    year = _NAMES[name]
    root, looked = find_year_dir(data_dir, year)
    if root is None:
        raise RuntimeError("%s (data_dir %r: no VOC%s folder with Annotations/ and JPEGImages/ at %s)" % (
            _UNAVAILABLE, str(data_dir), year, " or ".join(looked)))
    main = os.path.join(root, "ImageSets", "Main")
    entries = []
    for fname in _SPLIT_FILES[split]:
        path = os.path.join(main, fname)
        if not os.path.isfile(path):
            raise RuntimeError("%s (split %r of %s needs %s)" % (_UNAVAILABLE, split, name, path))
        entries += [(root, i) for i in _read_ids(path)]
    counts = {}
    for key, fname in (("train", "train.txt"), ("validation", "val.txt"), ("test", "test.txt")):
        path = os.path.join(main, fname)
        if os.path.isfile(path):
            counts[key] = len(_read_ids(path))
    return VocDataset(entries), VocInfo(name, root, counts)
