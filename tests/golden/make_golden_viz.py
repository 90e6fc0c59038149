"""Golden vectors for the colour images, produced by what the REFERENCE calls: np.percentile, matplotlib.colors.Normalize and
cm.ScalarMappable.to_rgba (KITTI/test_simple.py:166-172), and the reference's own colorize (NYUv2/utils.py:63-82) and
normalize_image (KITTI/utils.py:22-28).

The two modules cannot be imported here (imageio, skimage and six are absent), so -- as make_golden_dbe.py does -- this
script parses them, pulls the one function out with `ast` and executes exactly that definition.  colorize asks for
matplotlib.cm.get_cmap, which matplotlib 3.9 removed: it is bound to the registry that replaced it.  Run in the build
container only (numpy 2.2.6, matplotlib 3.10.8, torch on the CPU):

    python tests/golden/make_golden_viz.py            # writes tests/golden/viz_reference.npz
    python tests/golden/make_golden_viz.py --tables   # also wavelet_monodepth_amd/data/colormaps.json (CC0 colormap data, as hex text)

Per disparity case of tests/viz_cases.py: rgb [B,H,W,3] uint8 and range [B,2] float32 = (min, percentile); the resize cases
go through torch.nn.functional.interpolate on the CPU first, like the reference, and keep that map too (`resized`).  The
375 x 1242 case stores the range and the SHA-256 of the bytes.  Nothing from /root/reference is stored, and no inputs.
"""
import ast
import hashlib
import json
import os
import sys
import types

import matplotlib as mpl
import matplotlib.cm as cm
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viz_cases  # noqa: E402

REF = "/root/reference"


def extract(path, name, namespace):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            exec(compile(ast.Module([node], []), path, "exec"), namespace)
    return namespace[name]


def tables():
    return {n: (mpl.colormaps[n](np.arange(256))[:, :3] * 255).astype(np.uint8) for n in ("magma", "plasma")}


def disparity_image(disp_resized_np, q):
    vmax = np.percentile(disp_resized_np, q)
    normalizer = mpl.colors.Normalize(vmin=disp_resized_np.min(), vmax=vmax)
    mapper = cm.ScalarMappable(norm=normalizer, cmap="magma")
    return (mapper.to_rgba(disp_resized_np)[:, :, :3] * 255).astype(np.uint8), disp_resized_np.min(), vmax


def main():
    if "--tables" in sys.argv:
        os.makedirs(os.path.join(ROOT, "wavelet_monodepth_amd", "data"), exist_ok=True)
        doc = {"source": "matplotlib %s (colormap data CC0): (cmap(arange(256))[:, :3] * 255).astype(uint8), 256 rows of r g b, as hex"
                         % mpl.__version__}
        doc.update({k: v.tobytes().hex() for k, v in tables().items()})
        with open(os.path.join(ROOT, "wavelet_monodepth_amd", "data", "colormaps.json"), "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    shim = types.SimpleNamespace(cm=types.SimpleNamespace(get_cmap=lambda name: mpl.colormaps[name]))
    colorize = extract(os.path.join(REF, "NYUv2", "utils.py"), "colorize", {"matplotlib": shim, "np": np})
    normalize_image = extract(os.path.join(REF, "KITTI", "utils.py"), "normalize_image", {})
    out = {}
    for name in tuple(viz_cases.DISPARITY) + ("full",):
        case = viz_cases.disparity(name)
        x = torch.from_numpy(case["x"])[:, None]
        if case["size"] is not None:
            x = torch.nn.functional.interpolate(x, case["size"], mode="bilinear", align_corners=False)
        rgb, rng = [], []
        for b in range(x.shape[0]):
            im, lo, hi = disparity_image(x[b].squeeze(0).cpu().numpy(), case["q"])
            rgb.append(im)
            rng.append((lo, hi))
        rgb = np.stack(rgb)
        if name in viz_cases.RESIZED:
            out["disparity|%s|resized" % name] = x[:, 0].numpy()
        out["disparity|%s|range" % name] = np.array(rng, np.float32)
        assert np.array_equal(out["disparity|%s|range" % name].astype(np.float64), np.array(rng, np.float64)), name
        if name == "full":
            out["disparity|full|sha256"] = np.frombuffer(hashlib.sha256(rgb.tobytes()).digest(), np.uint8)
        else:
            out["disparity|%s|rgb" % name] = rgb
        print(name, rgb.shape, rng[0])
    for name in viz_cases.COLORIZE:
        case = viz_cases.colorize(name)
        with np.errstate(invalid="ignore"):
            out["colorize|%s" % name] = np.stack([colorize(torch.from_numpy(p)[None], case["vmin"], case["vmax"]) for p in case["x"]])
        print(name, out["colorize|%s" % name].shape)
    for name in viz_cases.NORMALIZE:
        case = viz_cases.normalize(name)
        x = torch.from_numpy(case["x"])
        y = torch.stack([normalize_image(p) for p in x]) if case["per_image"] else normalize_image(x)
        out["normalize|%s" % name] = y.numpy()
        print(name, y.shape)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "viz_reference.npz"), **out)


if __name__ == "__main__":
    main()
