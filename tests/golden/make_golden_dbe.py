"""Golden vectors for the NYUv2 depth-boundary errors, produced by the REFERENCE's own compute_depth_boundary_error.

NYUv2/utils.py cannot be imported here (skimage, cv2, matplotlib are absent), so this script parses it, pulls that one
function out with `ast` and executes exactly that definition with the real numpy and scipy.ndimage and with `feature.canny`
bound to tests/dbe_ref.py's detector: everything except the detector -- the normalisation, the distance transforms, the
truncation, the two scores -- is pinned by the reference's own code.  Run in the build container only:

    python tests/golden/make_golden_dbe.py        # writes tests/golden/dbe_reference.npz

Per case of tests/dbe_cases.py: the bit-packed edge maps, the two scores per image and the smallest decision margin
(dbe_ref.canny_stages) -- of the image the reference hands to the detector (it normalises in float32) and of the float64
normalisation this project defines, whichever is smaller.  Nothing from /root/reference is stored, and no inputs: the tests
regenerate them from wavelet_monodepth_amd.synth.
"""
import ast
import os
import sys
import types

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbe_cases  # noqa: E402
import dbe_ref  # noqa: E402

REF = "/root/reference"


def extract(path, names, namespace):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module([node], []), path, "exec"), namespace)
    missing = [n for n in names if n not in namespace]
    assert not missing, missing
    return namespace


class Detector:
    """stands in for skimage.feature: records the decision margin of every image it is handed"""

    def __init__(self):
        self.margins = []

    def canny(self, image, sigma, low_threshold, high_threshold):
        st = dbe_ref.canny_stages(image, sigma, low_threshold, high_threshold)
        self.margins.append(st["margin"])
        return st["edges"]


def main():
    det = Detector()
    ns = extract(os.path.join(REF, "NYUv2", "utils.py"), ["compute_depth_boundary_error"],
                 {"np": np, "ndimage": ndimage, "feature": types.SimpleNamespace(canny=det.canny)})
    ref = ns["compute_depth_boundary_error"]
    out = {}
    for name in dbe_cases.CASES:
        case = dbe_cases.build(name)
        B, H, W = case["pred"].shape
        scores, edges, margins = np.zeros((B, 2)), np.zeros((B, H, W), bool), np.full(B, np.inf)
        for b in range(B):
            gt = case["edges_gt"][b].astype(np.int64)
            if gt.sum() == 0:
                # the reference's first branch assigns (nan, nan) and then dies on its return statement (D_est is unbound)
                try:
                    ref(gt, case["pred"][b])
                    raise AssertionError("the reference returned without ground-truth edges")
                except UnboundLocalError:
                    scores[b] = np.nan
                continue
            det.margins = []
            mask = None if case["mask"] is None else case["mask"][b].astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                acc, com, e, _ = ref(gt, case["pred"][b], mask=mask, low_thresh=dbe_cases.LOW, high_thresh=dbe_cases.HIGH)
            scores[b], edges[b] = (acc, com), e
            own = dbe_ref.compute_depth_boundary_error(gt, case["pred"][b], mask, dbe_cases.LOW, dbe_cases.HIGH)
            margins[b] = min(det.margins + [own[3]])
        out[name + "|edges"] = np.packbits(edges)
        out[name + "|scores"] = scores
        out[name + "|margin"] = margins
        print(name, scores.round(4).tolist(), edges.sum((1, 2)).tolist(), margins)
    for name, H, W, sigma, low, high in dbe_cases.CANNY_CASES:
        st = dbe_ref.canny_stages(dbe_cases.canny_image(name, H, W), sigma, low, high)
        out[name + "|edges"] = np.packbits(st["edges"])
        out[name + "|margin"] = np.array([st["margin"]])
        print(name, int(st["edges"].sum()), st["margin"])
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "dbe_reference.npz"), **out)


if __name__ == "__main__":
    main()
