"""CPU tests of the VOC reader (``utils/voc_utils.py`` behind ``data_utils.get_dataset``) on a tiny devkit written with
Pillow at test time (tests/voc_cases.py), and the argument checks of ``ssd_preprocess_ragged`` (no device needed: every
check runs before any launch).  Expected boxes come from the chosen integers: float64 division, then float32, exact."""
import ctypes
import os

import numpy as np
import pytest

import ssd_hip
import voc_cases as vc
from utils import data_utils, voc_utils

pytest.importorskip("PIL")


@pytest.fixture(scope="module")
def devkit(tmp_path_factory):
    root = tmp_path_factory.mktemp("voc")
    vc.write_devkit(root, with_2012=True)
    return root


def test_annotations_parse_to_exact_boxes_labels_flags_in_xml_order(devkit):
    ds, _ = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    ids = vc.SPLITS_2007["train"] + vc.SPLITS_2007["val"]
    assert len(ds) == len(ids) == len(ds.records)
    for rec, image_id in zip(ds.records, ids):
        want = vc.expected_objects(image_id)
        assert rec["filename"] == image_id + ".jpg"
        assert rec["bbox"].dtype == np.float32 and rec["bbox"].shape == want["bbox"].shape
        assert np.array_equal(rec["bbox"].view(np.uint32), want["bbox"].view(np.uint32)), image_id
        assert rec["label"].dtype == np.int64 and np.array_equal(rec["label"], want["label"])
        assert rec["is_difficult"].dtype == bool and np.array_equal(rec["is_difficult"], want["is_difficult"])
        assert np.array_equal(rec["is_truncated"], want["is_truncated"])
    # spot values, written out: 000001's dog (48, 240, 195, 371) in a 375 x 500 image; no -1 offset
    dog = ds.records[0]["bbox"][0]
    assert dog.tolist() == [np.float32(240 / 375), np.float32(48 / 500), np.float32(371 / 375), np.float32(195 / 500)]
    assert ds.records[0]["label"].tolist() == [11, 14, 8]                      # dog, person, chair: alphabetical indices
    assert ds.records[0]["is_difficult"].tolist() == [False, False, True]
    # 000005 has no <difficult> tag at all
    assert ds.records[1]["filename"] == "000005.jpg" and ds.records[1]["is_difficult"].tolist() == [False, False]


def test_split_mapping_and_counts(devkit):
    for split, lists in [("train", ["train"]), ("validation", ["val"]), ("test", ["test"]),
                         ("train+validation", ["train", "val"])]:
        ds, info = data_utils.get_dataset("voc/2007", split, str(devkit))
        ids = sum([vc.SPLITS_2007[n] for n in lists], [])
        assert [r["filename"][:-4] for r in ds.records] == ids
        assert len(ds) == len(ids) == data_utils.get_total_item_size(info, split)
    assert info.splits["train"].num_examples == 4 and info.splits["validation"].num_examples == 3
    assert info.splits["test"].num_examples == 3
    assert data_utils.get_labels(info) == vc.CLASSES == data_utils.VOC_LABELS and len(data_utils.get_labels(info)) == 20
    with pytest.raises(AssertionError):
        data_utils.get_dataset("voc/2007", "trainval", str(devkit))


def test_data_dir_may_be_the_devkit_or_the_year_folder(devkit, monkeypatch):
    want = [r["filename"] for r in data_utils.get_dataset("voc/2007", "test", str(devkit))[0].records]
    for d in (devkit / "VOCdevkit", devkit / "VOCdevkit" / "VOC2007"):
        assert [r["filename"] for r in data_utils.get_dataset("voc/2007", "test", str(d))[0].records] == want
    monkeypatch.setenv("HOME", str(devkit))
    assert len(data_utils.get_dataset("voc/2007", "test", "~")[0]) == 3


def test_concatenate_covers_voc_2012(devkit):
    a, ia = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    b, ib = data_utils.get_dataset("voc/2012", "train+validation", str(devkit))
    both = a.concatenate(b)
    assert len(both) == 10 == data_utils.get_total_item_size(ia, "train+validation") + data_utils.get_total_item_size(
        ib, "train+validation")
    assert [r["filename"] for r in both.records] == [r["filename"] for r in a.records] + [r["filename"] for r in b.records]
    assert both.records[-1]["filename"] == "2008_000015.jpg"                  # train.txt then val.txt
    want = vc.expected_objects("2008_000008")
    assert np.array_equal(both.records[7]["bbox"].view(np.uint32), want["bbox"].view(np.uint32))
    assert voc_utils.has_year(str(devkit), "voc/2012")


def test_shuffle_is_a_seeded_permutation(devkit):
    a, _ = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    b, _ = data_utils.get_dataset("voc/2012", "train+validation", str(devkit))
    ds = a.concatenate(b)
    orders = {}
    for seed in (0, 1, 2, 3):
        first = ds.shuffle(4, seed=seed).order()
        assert sorted(first) == list(range(10))
        assert ds.shuffle(4, seed=seed).order() == first                       # reproducible per seed
        orders[seed] = tuple(first)
    assert len(set(orders.values())) > 1 and any(o != tuple(range(10)) for o in orders.values())
    # a buffer shuffle: item i cannot come out before position i - (buffer - 1)
    for o in orders.values():
        assert all(pos >= item - 3 for pos, item in enumerate(o))
    assert ds.shuffle(1, seed=5).order() == list(range(10))                    # a buffer of one keeps the order
    sh = ds.shuffle(10, seed=7)
    assert sh.order() != sh.order()                                            # a further pass draws a new order
    assert [r["filename"] for r in sh.iter_records()] != [] and len(sh) == 10
    assert [r["filename"] for r in ds.take(3).records] == [r["filename"] for r in ds.records[:3]]


def test_take_shard_and_concatenate_keep_their_state(devkit):
    a, _ = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    b, _ = data_utils.get_dataset("voc/2012", "train+validation", str(devkit))
    names = lambda d: [r["filename"] for r in d.records]
    for parsed in (False, True):                                               # before and after the annotations were parsed
        ds = a.concatenate(b)
        if parsed:
            want = names(ds)
        parts = [ds.shard(3, i) for i in range(3)]
        assert [len(p) for p in parts] == [4, 3, 3]
        want = names(a) + names(b)
        for i, p in enumerate(parts):
            assert names(p) == want[i::3]
        assert names(ds.take(4)) == want[:4] and names(ds.take(99)) == want and len(ds.take(0)) == 0
    sh = a.concatenate(b).shuffle(4, seed=2)
    first = a.concatenate(b).shuffle(4, seed=2).order()
    assert sh.take(10).order() == first and sorted(sh.shard(2, 1).order()) == list(range(5))   # the shuffle stays set
    assert sh.take(10).order() != list(range(10))
    with pytest.raises(ValueError):
        ds.shard(3, 3)
    with pytest.raises(ValueError, match="shuffle"):
        a.shuffle(4, seed=0).concatenate(b)
    with pytest.raises(ValueError, match="shuffle"):
        a.concatenate(b.shuffle(4, seed=0))


def test_missing_directory_split_file_and_unknown_class_raise(devkit, tmp_path, monkeypatch):
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    with pytest.raises(RuntimeError, match="tensorflow_datasets is not available") as e:
        data_utils.get_dataset("voc/2007", "test", str(tmp_path / "nowhere"))
    assert os.path.join(str(tmp_path / "nowhere"), "VOCdevkit", "VOC2007") in str(e.value)
    assert repr(str(tmp_path / "nowhere")) in str(e.value)                    # ... and the data_dir it was given
    (tmp_path / "VOC2007" / "Annotations").mkdir(parents=True)                # the year folder itself, no JPEGImages/
    with pytest.raises(RuntimeError) as e:
        data_utils.get_dataset("voc/2007", "test", str(tmp_path / "VOC2007"))
    assert repr(str(tmp_path / "VOC2007")) in str(e.value) and " or " in str(e.value)
    with pytest.raises(RuntimeError, match="tensorflow_datasets is not available"):
        data_utils.get_dataset("voc/2007", "test")                            # the default data_dir holds no devkit
    with pytest.raises(RuntimeError, match="tensorflow_datasets is not available") as e:
        data_utils.get_dataset("voc/2012", "test", str(devkit))               # VOC2012 here has no test.txt
    assert os.path.join("VOC2012", "ImageSets", "Main", "test.txt") in str(e.value)
    with pytest.raises(RuntimeError):
        data_utils.get_dataset("coco/2017", "train", str(devkit))
    vc.write_year(tmp_path, "2007", vc.IMAGES_2007[:2], {"train": ["000001", "000002"]})
    bad = tmp_path / "VOCdevkit" / "VOC2007" / "Annotations" / "000002.xml"
    bad.write_text(vc.xml_text("000002", 500, 375, "RGB", vc.IMAGES_2007[1][4], class_name="unicorn"))
    ds, _ = data_utils.get_dataset("voc/2007", "train", str(tmp_path))
    with pytest.raises(ValueError, match="000002.xml"):
        ds.records


def test_items_decode_to_what_pillow_decodes(devkit):
    ds, _ = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    ids = vc.SPLITS_2007["train"] + vc.SPLITS_2007["val"]
    items = list(ds)
    assert len(items) == len(ids)
    for item, image_id in zip(items, ids):
        _, h, w, _, _ = vc.spec(image_id)
        assert item["image"].dtype == np.uint8 and item["image"].shape == (h, w, 3)      # the grayscale file too
        assert np.array_equal(item["image"], vc.decoded(devkit, "2007", image_id))
        assert item["image/filename"] == image_id + ".jpg"
        want = vc.expected_objects(image_id)
        assert set(item["objects"]) == {"bbox", "label", "is_difficult", "is_truncated"}
        for k in want:
            assert np.array_equal(item["objects"][k], want[k])


def test_decoding_pool_size_is_never_the_cpu_count(monkeypatch):
    monkeypatch.delenv("SSD_DATA_WORKERS", raising=False)
    assert data_utils.data_workers() == 8
    assert data_utils.data_workers(3) == 3 and data_utils.data_workers(1000) == 16
    monkeypatch.setenv("SSD_DATA_WORKERS", "5")
    assert data_utils.data_workers() == 5 and data_utils.data_workers(2) == 2
    monkeypatch.setenv("SSD_DATA_WORKERS", "64")
    assert data_utils.data_workers() == 16


def test_preprocess_ragged_batch_rejects_wrong_dtype_and_rank_before_touching_the_device():
    for bad in (np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.uint8), np.zeros((1, 4, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            data_utils.preprocess_ragged_batch([bad], 20, 20)


def test_ssd_preprocess_ragged_argument_checks():
    """Every check runs on the host descriptors before any launch: the codes come back without a device."""
    l = ssd_hip.lib()
    one = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)        # a non-NULL stand-in; never dereferenced

    def call(desc_rows, src_bytes, B=None, C=3, oh=300, ow=300, src=one, ddev=one, out=one, host=True):
        desc = np.zeros(max(len(desc_rows), 1), ssd_hip.IMAGE_DESC_DTYPE)
        for i, (off, h, w) in enumerate(desc_rows):
            desc[i] = (off, h, w)
        return l.ssd_preprocess_ragged(src, src_bytes, desc.ctypes.data if host else None, ddev,
                                       len(desc_rows) if B is None else B, C, oh, ow, out, None)
    ok = [(0, 10, 10), (304, 5, 7)]
    assert call([], 0) == 0 and call([], 0, src=None, ddev=None, out=None, host=False) == 0      # B == 0: a no-op
    assert call(ok, 304 + 105, B=-1) == -1
    for kw in ({"src": None}, {"ddev": None}, {"out": None}, {"host": False}):                   # NULL pointers
        assert call(ok, 304 + 105, **kw) == -1, kw
    assert b"NULL" in l.ssd_last_error()
    assert call([(0, 10, 10), (300, 5, 7)], 4096) == -1                                          # offset not a multiple of 16
    assert call([(-16, 10, 10)], 4096) == -1
    assert call(ok, 304 + 104) == -1                                                             # one byte short
    assert b"outside the source buffer" in l.ssd_last_error()
    assert call([(0, 16384, 16384)], 16384 * 16384 * 3 - 1) == -1
    for kw in ({"C": 4}, {"C": 1}, {"oh": 0}, {"ow": 16385}, {"B": 65536}):
        assert call(ok, 4096, **kw) == -3, kw
    for rows in ([(0, 0, 10)], [(0, 10, 0)], [(0, 16385, 1)], [(0, 10, 10), (304, 1, 16385)]):
        assert call(rows, 1 << 40) == -3, rows
    assert isinstance(l.ssd_last_error(), bytes)
