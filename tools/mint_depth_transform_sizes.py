"""Mints tests/golden/depth_transform_sizes.json: what the reference's own Resize.get_size (depth_anything/util/transform.py:109-166) returns
for a table of inputs, the yardstick of diffreg_hip.depth_transform2d3d.transform_size.

    python tools/mint_depth_transform_sizes.py --reference <a Diff-Reg-2d3d checkout>

The reference's module is loaded from where it lies with cv2, torchvision and PIL stubbed in sys.modules (get_size needs none of them; only the
interpolation constants are read at import).  Runs where a checkout exists; no test imports this file.
"""
import argparse
import importlib.util
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (width, height, target_width, target_height, multiple_of, keep_aspect_ratio, resize_method)
TABLE = [
    (640, 480, 630, 476, 14, True, "lower_bound"),          # production: -> (630, 476)
    (637, 476, 630, 476, 14, True, "lower_bound"),          # 637 / 14 = 45.5: half to even -> 46 -> 644
    (651, 476, 630, 476, 14, True, "lower_bound"),          # 651 / 14 = 46.5: half to even -> 46 -> 644
    (480, 640, 630, 476, 14, True, "lower_bound"),          # portrait
    (100, 50, 630, 476, 14, True, "lower_bound"),           # small
    (1241, 376, 630, 476, 14, True, "lower_bound"),         # wide
    (640, 480, 518, 518, 14, True, "lower_bound"),
    (640, 480, 645, 480, 14, True, "lower_bound"),          # 645 / 14 = 46.07 rounds to 644 < min_val: the ceil branch -> 658
    (645, 480, 630, 476, 14, True, "upper_bound"),
    (640, 480, 630, 476, 14, True, "upper_bound"),
    (500, 500, 630, 476, 14, True, "upper_bound"),
    (640, 480, 640, 485, 14, True, "upper_bound"),          # 485 / 14 = 34.64 rounds to 490 > max_val: the floor branch -> 476
    (640, 480, 640, 485, 14, False, "upper_bound"),         # the same branch on both axes
    (1000, 30, 630, 476, 14, True, "upper_bound"),
    (640, 480, 630, 476, 14, True, "minimal"),              # (minimal passes min_val = 0 and no max_val: neither branch can be taken)
    (600, 470, 630, 476, 14, True, "minimal"),
    (9, 7, 630, 476, 14, True, "minimal"),
    (2000, 5, 630, 476, 14, True, "minimal"),               # 1.575 rows round to 0: y = min_val, still not below it
    (640, 480, 630, 476, 14, False, "lower_bound"),         # keep_aspect_ratio=False
    (333, 777, 630, 476, 14, False, "upper_bound"),
    (333, 777, 630, 476, 14, False, "minimal"),
    (640, 480, 630, 476, 1, True, "lower_bound"),           # multiple_of = 1
    (641, 479, 630, 476, 32, True, "lower_bound"),
    (40, 30, 42, 28, 14, True, "lower_bound"),              # the shapes of the GPU tests
    (64, 48, 42, 28, 14, True, "lower_bound"),
]


def load_resize(reference):
    for name in ("cv2", "torchvision", "torchvision.transforms", "PIL", "PIL.Image", "PIL.ImageOps", "PIL.ImageFilter"):
        sys.modules[name] = types.ModuleType(name)
    cv2 = sys.modules["cv2"]
    cv2.INTER_AREA, cv2.INTER_CUBIC, cv2.INTER_NEAREST = 3, 2, 0
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    for sub in ("Image", "ImageOps", "ImageFilter"):
        setattr(sys.modules["PIL"], sub, sys.modules["PIL." + sub])
    path = os.path.join(reference, "depth_anything", "util", "transform.py")
    spec = importlib.util.spec_from_file_location("_reference_transform", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Resize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a Diff-Reg-2d3d checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "depth_transform_sizes.json"))
    a = ap.parse_args()
    Resize = load_resize(a.reference)
    rows = []
    for width, height, tw, th, m, keep, method in TABLE:
        r = Resize(width=tw, height=th, resize_target=False, keep_aspect_ratio=keep, ensure_multiple_of=m, resize_method=method)
        new_w, new_h = r.get_size(width, height)
        rows.append(dict(width=width, height=height, target_width=tw, target_height=th, multiple_of=m, keep_aspect_ratio=keep, resize_method=method,
                         new_width=int(new_w), new_height=int(new_h)))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print("wrote %d rows to %s" % (len(rows), a.out))


if __name__ == "__main__":
    main()
