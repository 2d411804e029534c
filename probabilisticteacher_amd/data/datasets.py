"""Dataset registry, the Pascal-VOC directory reader (reference pt/data/datasets/builtin.py:118-149: every dataset of the
shipped configs is a VOC-format directory registered under a name; detectron2's `register_pascal_voc` /
`load_voc_instances` do the reading there) and the COCO-format json reader (builtin.py:27-116; the reference's defaults,
DATASETS.TRAIN_LABEL = coco_2017_train and TEST.EVALUATOR = COCOeval, are COCO).

Host side of the boundary: XML parsing and image decoding (Pillow) happen here; everything after the decoded uint8 tensor is
the device pipeline of data/mapper.py."""
import os
import xml.etree.ElementTree as ET
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

_DATASETS: Dict[str, Callable[[], List[dict]]] = {}
_METADATA: Dict[str, dict] = {}

CLASS_NAMES = {        # builtin.py:134-147
    1: ("car",),
    7: ("truck", "car", "rider", "person", "motorcycle", "bicycle", "bus"),
    8: ("truck", "car", "rider", "person", "train", "motorcycle", "bicycle", "bus"),
    20: ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse",
         "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"),
}
VOC_SPLITS = [         # builtin.py:120-130: (name, directory under the dataset root, split, number of classes)
    ("VOC2007_citytrain", "data/VOC2007_citytrain", "train", 8), ("VOC2007_foggytrain", "data/VOC2007_foggytrain", "train", 8),
    ("VOC2007_foggyval", "data/VOC2007_foggyval", "val", 8), ("VOC2007_citytrain1", "data/VOC2007_citytrain1", "train", 1),
    ("VOC2007_cityval1", "data/VOC2007_cityval1", "val", 1), ("VOC2007_bddtrain", "data/VOC2007_bddtrain", "train", 8),
    ("VOC2007_bddval", "data/VOC2007_bddval", "val", 8), ("VOC2007_kitti1", "data/kitti", "train", 1),
    ("VOC2007_sim1", "data/sim", "train", 1),
]


def load_voc_instances(dirname: str, split: str, class_names: Sequence[str]) -> List[dict]:
    """D2 load_voc_instances: ImageSets/Main/<split>.txt lists the ids; Annotations/<id>.xml, JPEGImages/<id>.jpg.  The XML's
    1-based inclusive corners become 0-based boxes by subtracting 1 from xmin / ymin only (D2's convention, which the
    evaluator undoes)."""
    with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
        ids = [line.strip() for line in f if line.strip()]
    dicts = []
    for fid in ids:
        tree = ET.parse(os.path.join(dirname, "Annotations", fid + ".xml"))
        rec = {"file_name": os.path.join(dirname, "JPEGImages", fid + ".jpg"), "image_id": fid,
               "height": int(tree.findall("./size/height")[0].text), "width": int(tree.findall("./size/width")[0].text)}
        ann = []
        for obj in tree.findall("object"):
            name = obj.find("name").text
            if name not in class_names:
                continue
            bb = obj.find("bndbox")
            box = [float(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")]
            box[0] -= 1.0
            box[1] -= 1.0
            diff = obj.find("difficult")
            ann.append({"category_id": class_names.index(name), "bbox": box, "difficult": int(diff.text) if diff is not None else 0})
        rec["annotations"] = ann
        dicts.append(rec)
    return dicts


def register_pascal_voc(name: str, dirname: str, split: str, class_names: Sequence[str], year: int = 2012) -> None:
    _DATASETS[name] = lambda: load_voc_instances(dirname, split, class_names)
    _METADATA[name] = {"thing_classes": list(class_names), "dirname": dirname, "split": split, "year": year,
                       "evaluator_type": "pascal_voc"}


def register_all_pascal_voc(root: str) -> None:
    for name, d, split, ncls in VOC_SPLITS:
        register_pascal_voc(name, os.path.join(root, d), split, CLASS_NAMES[ncls])


COCO_SPLITS = {        # builtin.py:29-38: name -> (image root, json file) under the dataset root
    "coco_2017_unlabel": ("coco/unlabeled2017", "coco/annotations/image_info_unlabeled2017.json"),
    "coco_2017_for_voc20": ("coco", "coco/annotations/google/instances_unlabeledtrainval20class.json"),
}


def _coco_categories(data: dict):
    """thing_classes and dataset id -> contiguous id, by ascending dataset id (D2 load_coco_json); (None, None) without
    categories (image_info_*.json)"""
    cats = sorted(data.get("categories", []), key=lambda c: c["id"])
    if not cats:
        return None, None
    return [c["name"] for c in cats], {c["id"]: i for i, c in enumerate(cats)}


def load_coco_json(json_file: str, image_root: str) -> List[dict]:
    """D2 load_coco_json / the reference's load_coco_unlabel_json (builtin.py:83-116) with plain `json`: one record per image,
    images sorted by id (builtin.py:99).  Annotations: category_id contiguous, "bbox" XYXY (this repository's convention;
    x + w, y + h in double), "bbox_xywh" as the file has it (what the COCO evaluator scores against), iscrowd, area (w * h where
    the file has none).  A json without an `annotations` key (coco_2017_unlabel) yields records without `annotations`."""
    import json
    with open(json_file) as f:
        data = json.load(f)
    _, id_map = _coco_categories(data)
    per_image = None
    if "annotations" in data:
        per_image = {}
        for a in data["annotations"]:
            per_image.setdefault(a["image_id"], []).append(a)
    dicts = []
    for img in sorted(data["images"], key=lambda i: i["id"]):
        rec = {"file_name": os.path.join(image_root, img["file_name"]), "height": img["height"], "width": img["width"],
               "image_id": img["id"]}
        if per_image is not None:
            ann = []
            for a in per_image.get(img["id"], []):
                x, y, w, h = (float(v) for v in a["bbox"])
                ann.append({"category_id": id_map[a["category_id"]], "bbox": [x, y, x + w, y + h], "bbox_xywh": [x, y, w, h],
                            "iscrowd": int(a.get("iscrowd", 0)), "area": float(a["area"]) if "area" in a else w * h})
            rec["annotations"] = ann
        dicts.append(rec)
    return dicts


def register_coco_instances(name: str, json_file: str, image_root: str) -> None:
    """builtin.py:50-80.  thing_classes / thing_dataset_id_to_contiguous_id are read from the json the first time the
    metadata is asked for, so registering a split whose files are absent costs nothing."""
    _DATASETS[name] = lambda: load_coco_json(json_file, image_root)
    _METADATA[name] = {"json_file": json_file, "image_root": image_root, "evaluator_type": "coco"}


def register_coco_unlabel(root: str) -> None:
    for name, (image_root, json_file) in COCO_SPLITS.items():       # builtin.py:41-47
        register_coco_instances(name, os.path.join(root, json_file), os.path.join(root, image_root))


def get_dataset_dicts(names: Sequence[str], filter_empty: bool = False) -> List[dict]:
    """D2 get_detection_dataset_dicts: concatenation of the named datasets, optionally without annotation-less images"""
    out = []
    for n in names:
        if n not in _DATASETS:
            raise KeyError(f"dataset {n!r} is not registered (register_pascal_voc / DETECTRON2_DATASETS)")
        d = _DATASETS[n]()
        assert len(d), f"dataset {n!r} is empty"
        out += d
    if filter_empty:
        out = [d for d in out if len(d.get("annotations", []))]
    return out


def metadata(name: str) -> dict:
    m = _METADATA[name]
    if m.get("evaluator_type") == "coco" and "thing_classes" not in m:
        import json
        with open(m["json_file"]) as f:
            names, id_map = _coco_categories(json.load(f))
        m.update(thing_classes=names or [], thing_dataset_id_to_contiguous_id=id_map or {})
    return m


def read_image_hwc(file_name: str) -> np.ndarray:
    """the decode of detection_utils.read_image alone: uint8 (H, W, 3) RGB, upright, as Pillow delivers it.  This is what
    the loader's decode workers run (data/prefetch.py looks it up per call)."""
    from PIL import Image, ImageOps
    with Image.open(file_name) as im:
        im = ImageOps.exif_transpose(im)          # D2 _apply_exif_orientation: rotated JPEGs are turned upright
        return np.asarray(im.convert("RGB"))


def read_image(file_name: str, fmt: str = "BGR") -> torch.Tensor:
    """detection_utils.read_image + the mapper's HWC -> CHW transpose (dataset_mapper.py:162-169): uint8 (3, H, W)"""
    from PIL import Image, ImageOps
    with Image.open(file_name) as im:
        im = ImageOps.exif_transpose(im)          # D2 _apply_exif_orientation: rotated JPEGs are turned upright
        arr = np.asarray(im.convert("RGB"))
    if fmt == "BGR":
        arr = arr[:, :, ::-1]
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def to_mapper_input(d: dict, fmt: str = "BGR", image: Optional[torch.Tensor] = None, is_train: bool = True) -> dict:
    """dataset dict -> what DeviceTwoCropMapper takes: decoded image + boxes / classes (+ difficult flags).  `image`: the
    already decoded uint8 (3, H, W) image in `fmt` order (the decode-ahead path); None: read it here.  is_train: crowd
    annotations (COCO `iscrowd`) are dropped, as D2's DatasetMapper does for training; False (test records): they stay and
    `iscrowd` / `area` ride along where the dataset has them, for the COCO evaluator.  VOC dicts have neither key."""
    out = {"image": read_image(d["file_name"], fmt) if image is None else image, "image_id": d["image_id"],
           "file_name": d["file_name"]}
    ann = d.get("annotations")
    if ann is not None:
        if is_train:
            ann = [a for a in ann if a.get("iscrowd", 0) == 0]
        else:
            if any("iscrowd" in a for a in ann):
                out["iscrowd"] = torch.tensor([a.get("iscrowd", 0) for a in ann], dtype=torch.int32)
            if ann and all("area" in a for a in ann):
                out["area"] = torch.tensor([a["area"] for a in ann], dtype=torch.float64)
        out["boxes"] = torch.tensor([a["bbox"] for a in ann], dtype=torch.float32).reshape(-1, 4)
        out["classes"] = torch.tensor([a["category_id"] for a in ann], dtype=torch.int64)
        out["difficult"] = torch.tensor([a.get("difficult", 0) for a in ann], dtype=torch.bool)
    return out


register_coco_unlabel(os.getenv("DETECTRON2_DATASETS", ""))        # builtin.py:152-154
register_all_pascal_voc(os.getenv("DETECTRON2_DATASETS", ""))
