"""Golden vectors for the KITTI training inputs, produced by the REFERENCE's own MonoDataset.preprocess over Pillow.

KITTI/datasets/mono_dataset.py cannot be imported here (cv2 and torchvision are absent), so this script parses it, pulls
`MonoDataset.preprocess` out with `ast` and executes exactly that definition on real PIL images.  The stand-ins for the
absent torchvision pieces are each a thin call into Pillow:

    T.Resize((h, w), ANTIALIAS)   img.resize((w, h), Image.LANCZOS)
    T.ToTensor()                  float32 CHW, np.asarray(img) / 255
    ColorJitter.get_params(...)   ImageEnhance.Brightness / Contrast / Color and the HSV hue shift of torchvision 0.8.2's
                                  adjust_hue (np_h += np.uint8(hue_factor * 255)), composed in the case's order
    get_color's flip              img.transpose(Image.FLIP_LEFT_RIGHT)

Run in the build container only:

    python tests/golden/make_golden_inputs.py        # writes tests/golden/inputs_reference.npz

Stored per case of tests/inputs_cases.py and scale s: "<name>|color|<s>" and "<name>|aug|<s>", uint8 [N,h,w,3] (the
tensors times 255, asserted to divide back exactly); "pillow" the version; "cube|<shift>" the SHA-256 of Pillow's
RGB -> HSV, H += shift, -> RGB over all 2^24 colours.  Asserted here, so that a fixture that contradicts
tests/inputs_ref.py cannot be written: oracle == Pillow on every case, every cube, both colour conversions over the
cube, and the three blends at five factors.  Nothing from the reference is stored, and no inputs.
"""
import ast
import hashlib
import os
import sys
import types

import numpy as np
import PIL
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inputs_cases  # noqa: E402
import inputs_ref as R  # noqa: E402

REF = "/root/reference/KITTI/datasets/mono_dataset.py"


def extract_preprocess():
    tree = ast.parse(open(REF).read())
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == "MonoDataset":
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and fn.name == "preprocess":
                    ns = {}
                    exec(compile(ast.Module([fn], []), REF, "exec"), ns)
                    return ns["preprocess"]
    raise AssertionError("MonoDataset.preprocess not found")


def pil_hue(img, shift):
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(shift)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_jitter(order, factors, shift):
    ops = [lambda im: ImageEnhance.Brightness(im).enhance(float(factors[0])),
           lambda im: ImageEnhance.Contrast(im).enhance(float(factors[1])),
           lambda im: ImageEnhance.Color(im).enhance(float(factors[2])),
           lambda im: pil_hue(im, int(shift))]

    def apply(im):
        for op in order:
            im = ops[int(op)](im)
        return im
    return apply


def to_tensor(img):
    return np.ascontiguousarray((np.asarray(img).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def back_to_u8(t):
    u8 = np.rint(t.transpose(1, 2, 0).astype(np.float64) * 255.0).astype(np.uint8)
    assert np.array_equal(R.to_tensor(u8), t)
    return u8


def reference_item(preprocess, case, i):
    S = case["num_scales"]
    me = types.SimpleNamespace(num_scales=S, target_scales=list(range(S)), to_tensor=to_tensor, resize={})
    for s in range(S):
        size = (case["width"] // 2 ** s, case["height"] // 2 ** s)
        me.resize[s] = lambda im, size=size: im.resize(size, Image.LANCZOS)
    img = Image.fromarray(case["frames"][i], "RGB")
    if case["flip"][i]:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    j = case["jitter"]
    aug = pil_jitter(j["order"][i], j["factors"][i], j["hue_shift"][i]) if j is not None and j["enable"][i] else (lambda x: x)
    inputs = {("color", 0, -1): img}
    preprocess(me, inputs, aug)
    return ([back_to_u8(inputs[("color", 0, s)]) for s in range(S)], [back_to_u8(inputs[("color_aug", 0, s)]) for s in range(S)])


def oracle_item(case, i):
    levels = R.pyramid(case["frames"][i], case["height"], case["width"], case["num_scales"], bool(case["flip"][i]))
    j = case["jitter"]
    if j is None or not j["enable"][i]:
        return levels, levels
    return levels, [R.jitter(l, j["order"][i], j["factors"][i], j["hue_shift"][i]) for l in levels]


def check_primitives(cube):
    img = Image.fromarray(cube, "RGB")
    hsv = np.asarray(img.convert("HSV"))
    assert np.array_equal(R.rgb_to_hsv(cube), hsv), "rgb_to_hsv differs from Pillow"
    assert np.array_equal(R.hsv_to_rgb(cube), np.asarray(Image.fromarray(cube, "HSV").convert("RGB"))), "hsv_to_rgb differs from Pillow"
    small = inputs_cases.image("blend", (64, 96, 3), 9)
    pim = Image.fromarray(small, "RGB")
    for f in (0.8, 0.93, 1.0, 1.07, 1.2):
        assert np.array_equal(R.brightness(small, f), np.asarray(ImageEnhance.Brightness(pim).enhance(f))), f
        assert np.array_equal(R.contrast(small, f), np.asarray(ImageEnhance.Contrast(pim).enhance(f))), f
        assert np.array_equal(R.saturation(small, f), np.asarray(ImageEnhance.Color(pim).enhance(f))), f
    for (a, b) in [(1242, 640), (375, 192), (37, 16), (14, 24)]:
        src = inputs_cases.image("tab", (3, a, 3), 5)
        assert np.array_equal(R.resize(src, 3, b), np.asarray(Image.fromarray(src, "RGB").resize((b, 3), Image.LANCZOS))), (a, b)
    print("primitives: both colour conversions over 2^24 colours, three blends at five factors, four resizes: equal")


def main():
    preprocess = extract_preprocess()
    out = {"pillow": np.array(PIL.__version__)}
    cube = R.colour_cube()
    check_primitives(cube)
    for shift in inputs_cases.CUBE_SHIFTS:
        ref = np.asarray(pil_hue(Image.fromarray(cube, "RGB"), shift))
        assert np.array_equal(R.hue(cube, shift), ref), shift
        out["cube|%d" % shift] = np.array(hashlib.sha256(ref.tobytes()).hexdigest())
        print("cube shift %3d: %d colours moved, sha256 %s" % (shift, int((ref != cube).any(-1).sum()), out["cube|%d" % shift]))
    for name in inputs_cases.CASES:
        case = inputs_cases.build(name)
        N, S = len(case["frames"]), case["num_scales"]
        color, aug = [[] for _ in range(S)], [[] for _ in range(S)]
        for i in range(N):
            rc, ra = reference_item(preprocess, case, i)
            oc, oa = oracle_item(case, i)
            for s in range(S):
                assert np.array_equal(rc[s], oc[s]), (name, i, s, "color")
                assert np.array_equal(ra[s], oa[s]), (name, i, s, "aug")
                color[s].append(rc[s])
                aug[s].append(ra[s])
        for s in range(S):
            out["%s|color|%d" % (name, s)] = np.stack(color[s])
            out["%s|aug|%d" % (name, s)] = np.stack(aug[s])
        print("%-16s N %2d  %s  oracle == Pillow" % (name, N, [out["%s|color|%d" % (name, s)].shape[1:3] for s in range(S)]))
    path = os.path.join(ROOT, "tests", "golden", "inputs_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes (Pillow %s)" % (path, os.path.getsize(path), PIL.__version__))


if __name__ == "__main__":
    main()
