"""Golden vectors for the NYUv2 training inputs, produced by the REFERENCE's own transforms over Pillow.

NYUv2/data.py cannot be imported here (torchvision and sklearn are absent), so this script parses it, pulls
`RandomHorizontalFlip`, `RandomChannelSwap`, `RandomGamma` and `ToTensor` (and the two `_is_*_image` helpers they call) out
with `ast` and executes exactly those definitions on real PIL images.  The stand-ins for what is absent or rotted are thin:

    TF.adjust_gamma(img, g, gain)   torchvision's documented PIL path: img.point([(255 + 1 - 1e-3) * gain * pow(e / 255., g)] * 3)
    random                          a scripted object: random() / randint() / uniform() return the case's draws
    ToTensor.to_tensor              only if torch.ByteStorage.from_buffer no longer runs: uint8 HWC -> float CHW / 255

The reference's crop box and sizes are hard-coded, so only the 480 x 640 cases (`real_*`) go through its classes; the small
cases run the same Pillow calls (transpose, fromarray of the permuted array, point, crop, resize) with the case's box and
sizes.  Run in the build container only:

    python tests/golden/make_golden_nyu_inputs.py <reference>/NYUv2/data.py        # writes tests/golden/nyu_inputs_reference.npz

Stored per case of tests/nyu_inputs_cases.py: small cases "<name>|image" uint8 [N,ih,iw,3] and "<name>|depth" uint8
[N,dh,dw]; `real_*` cases per item i "<name>|image_sha|<i>" (SHA-256 of the uint8 image bytes, HWC), "<name>|depth_sha|<i>"
(SHA-256 of the float32 depth tensor's bytes) and "<name>|image_sub|<i>" / "<name>|depth_sub|<i>", every eighth row and column
as uint8; "gamma|<g>" the tables at 0.8 / 1.0 / 1.25 as Image.point applied them; "pillow" the version.  Asserted here, so that
a fixture that contradicts tests/nyu_inputs_ref.py cannot be written: oracle == Pillow on every case, and the bicubic table ==
Image.resize on single rows for every (in, out) pair of the cases.  Nothing from the reference is stored, and no inputs.
"""
import ast
import hashlib
import os
import sys
import types

import numpy as np
import PIL
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nyu_inputs_cases as cases  # noqa: E402
import nyu_inputs_ref as R  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(sys.argv[1]):
    sys.exit("usage: make_golden_nyu_inputs.py <the reference's NYUv2/data.py>")
REF = sys.argv[1]
WANTED = ("_is_pil_image", "_is_numpy_image", "RandomHorizontalFlip", "RandomChannelSwap", "RandomGamma", "ToTensor")


def adjust_gamma(img, gamma, gain=1):
    input_mode = img.mode
    img = img.convert("RGB")
    gamma_map = [(255 + 1 - 1e-3) * gain * pow(ele / 255., gamma) for ele in range(256)] * 3
    return img.point(gamma_map).convert(input_mode)


class Script:
    """random.random / randint / uniform in the order the three transforms call them"""

    def __init__(self, draws):
        self.draws = list(draws)

    def _next(self, kind):
        k, v = self.draws.pop(0)
        assert k == kind, (k, kind)
        return v

    def random(self):
        return self._next("random")

    def randint(self, a, b):
        v = self._next("randint")
        assert a <= v <= b
        return v

    def uniform(self, a, b):
        v = self._next("uniform")
        assert min(a, b) <= v <= max(a, b)
        return v


def extract():
    tree = ast.parse(open(REF).read())
    nodes = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in WANTED]
    assert sorted(n.name for n in nodes) == sorted(WANTED)
    ns = {"np": np, "torch": torch, "Image": Image, "TF": types.SimpleNamespace(adjust_gamma=adjust_gamma)}
    exec(compile(ast.Module(nodes, []), REF, "exec"), ns)
    try:
        ns["ToTensor"]().to_tensor(Image.fromarray(np.zeros((2, 2, 3), np.uint8), "RGB"))
        print("ToTensor.to_tensor: the reference's own")
    except Exception as e:  # torch.ByteStorage.from_buffer
        print("ToTensor.to_tensor: stand-in (%s: %s)" % (type(e).__name__, e))

        def to_tensor(self, pic):
            a = np.asarray(pic)
            a = a[..., None] if a.ndim == 2 else a
            return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float().div(255)
        ns["ToTensor"].to_tensor = to_tensor
    return ns


def reference_item(ns, c, i):
    """item i of a 480 x 640 case through the reference's classes -> (image float32 [3,h,w], depth float32 [1,h,w])"""
    draws = [("random", 0.0 if c["flip"][i] else 0.9)]
    draws += [("random", 0.0), ("randint", int(c["perm"][i]))] if c["perm"][i] else [("random", 0.9)]
    if c["gamma"][i] is not None:
        draws.append(("uniform", float(c["gamma"][i])))
    script = Script(draws)
    ns["random"] = script
    sample = {"image": Image.fromarray(c["image"][i], "RGB"), "depth": Image.fromarray(c["depth"][i], "L")}
    for t in (ns["RandomHorizontalFlip"](), ns["RandomChannelSwap"](0.1), ns["RandomGamma"](0.8 if c["gamma"][i] is not None else 0),
              ns["ToTensor"](is_224=c["is_224"])):
        sample = t(sample)
    assert not script.draws
    return sample["image"].numpy(), sample["depth"].numpy()


def pillow_item(c, i):
    """the same Pillow calls with the case's box and sizes -> (image u8 [ih,iw,3], depth u8 [dh,dw])"""
    image, depth = Image.fromarray(c["image"][i], "RGB"), Image.fromarray(c["depth"][i], "L")
    if c["flip"][i]:
        image, depth = image.transpose(Image.FLIP_LEFT_RIGHT), depth.transpose(Image.FLIP_LEFT_RIGHT)
    if c["perm"][i]:
        image = Image.fromarray(np.asarray(image)[..., list(R.PERMS[int(c["perm"][i])])])
    if c["gamma"][i] is not None:
        image = adjust_gamma(image, float(c["gamma"][i]), gain=1)
    H0, W0 = c["image"].shape[1:3]
    k = c["crop"]
    box = (k, k, W0 - k, H0 - k)
    (ih, iw), (dh, dw) = c["image_size"], c["depth_size"]
    return np.asarray(image.crop(box).resize((iw, ih))), np.asarray(depth.crop(box).resize((dw, dh)))


def check_tables():
    for a, b in cases.table_pairs():
        src = cases.noise("tab", (3, a, 1), 5)
        want = np.asarray(Image.fromarray(src[..., 0], "L").resize((b, 3), Image.BICUBIC))
        assert np.array_equal(R.resize(src, 3, b)[..., 0], want), (a, b)
    print("bicubic tables: %d (in, out) pairs equal Image.resize on single rows" % len(cases.table_pairs()))


def main():
    assert Image.new("L", (4, 4)).resize((2, 2)).tobytes() == Image.new("L", (4, 4)).resize((2, 2), Image.BICUBIC).tobytes()
    ns = extract()
    check_tables()
    out = {"pillow": np.array(PIL.__version__)}
    for g in (0.8, 1.0, 1.25):
        ramp = Image.fromarray(np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2), "RGB")
        tab = np.asarray(adjust_gamma(ramp, g))[..., 0].ravel()
        assert np.array_equal(tab, R.gamma_lut(g)), g
        out["gamma|%s" % g] = tab
    for name in cases.CASES:
        c = cases.build(name)
        n = len(c["image"])
        images, depths = [], []
        for i in range(n):
            pi, pd = pillow_item(c, i)
            oi, od = cases.oracle(c, i)
            assert np.array_equal(pi, oi), (name, i, "image")
            assert np.array_equal(pd, od), (name, i, "depth")
            if name in cases.REAL:
                ri, rd = reference_item(ns, c, i)
                assert ri.dtype == np.float32 and rd.dtype == np.float32
                assert np.array_equal(ri, R.image_tensor(pi)), (name, i, "reference image")
                assert np.array_equal(rd, R.depth_tensor(pd)), (name, i, "reference depth")
                out["%s|image_sha|%d" % (name, i)] = np.array(hashlib.sha256(np.ascontiguousarray(pi).tobytes()).hexdigest())
                out["%s|depth_sha|%d" % (name, i)] = np.array(hashlib.sha256(np.ascontiguousarray(rd).tobytes()).hexdigest())
                out["%s|image_sub|%d" % (name, i)] = np.ascontiguousarray(pi[::8, ::8])
                out["%s|depth_sub|%d" % (name, i)] = np.ascontiguousarray(pd[::8, ::8])
            images.append(pi)
            depths.append(pd)
        if name in cases.SMALL:
            out[name + "|image"], out[name + "|depth"] = np.stack(images), np.stack(depths)
        print("%-16s N %d  image %s depth %s  oracle == Pillow%s" % (name, n, images[0].shape[:2], depths[0].shape,
                                                                    " == the reference's classes" if name in cases.REAL else ""))
    path = os.path.join(ROOT, "tests", "golden", "nyu_inputs_reference.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 400000, size
    print("wrote %s: %d bytes (Pillow %s)" % (path, size, PIL.__version__))


if __name__ == "__main__":
    main()
