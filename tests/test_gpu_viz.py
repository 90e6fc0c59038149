"""GPU: the colour images (csrc/wmd_viz.hip through wavelet_monodepth_amd.visualize) against tests/golden/viz_reference.npz,
which np.percentile, matplotlib and the reference's own colorize / normalize_image wrote: bytes for bytes, ranges by value.
Where a case resizes, the map itself is pinned bit for bit to ops.upsample_bilinear and the colours to viz_ref on that map;
against the fixture, whose map ATen resampled on the CPU, such a case holds to the resample's rounding
(viz_ref.assert_resampled_close).  Reads the fixture only."""
import hashlib

import numpy as np
import pytest
import torch

import viz_cases
import viz_ref
from util import load_golden
from wavelet_monodepth_amd import ops, visualize as viz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return load_golden("viz_reference.npz")


@pytest.fixture(scope="module")
def magma():
    return viz_ref.table("magma")


def run(case, dev, **kw):
    x = torch.from_numpy(case["x"]).to(dev)
    rgb, rng, res = viz.disparity_image(x, case["size"], case["q"], return_range=True, return_resized=True, **kw)
    assert rgb.dtype == torch.uint8 and rgb.is_cuda and tuple(rgb.shape) == tuple(res.shape) + (3,)
    return x, rgb.cpu().numpy(), rng.cpu().numpy(), res


@pytest.mark.parametrize("name", tuple(viz_cases.DISPARITY))
def test_disparity_image_vs_fixture(dev, gold, magma, name):
    """n = 1, 2, 3; q = 0, 60, 95, 99.5, 100; constant, duplicates at the percentile, narrow, heavy-tailed, signed; ragged
    sizes; B = 3 with a constant image in the middle; the three resize cases (two blocks per image at 47 x 155)"""
    case = viz_cases.disparity(name)
    x, rgb, rng, res = run(case, dev)
    B, h, w = case["x"].shape
    H, W = case["size"] or (h, w)
    # the map: the existing resample, bit for bit (the identity when the size does not change)
    want_map = ops.upsample_bilinear(x[:, None], (H, W))[:, 0] if (H, W) != (h, w) else x
    assert torch.equal(res.view(torch.int32), want_map.contiguous().view(torch.int32)), name
    res = res.cpu().numpy()
    for b in range(B):
        # the colours and the range: the numpy rules on that very map
        own_rgb, lo, hi = viz_ref.disparity_image(res[b], case["q"], magma)
        print(name, b, "range", rng[b].tolist(), "viz_ref", (float(lo), float(hi)), "fixture", gold["disparity|%s|range" % name][b].tolist(),
              "pixels off viz_ref", int((rgb[b] != own_rgb).any(-1).sum()), "off fixture", int((rgb[b] != gold["disparity|%s|rgb" % name][b]).any(-1).sum()))
        assert (rng[b, 0], rng[b, 1]) == (lo, hi), (name, b)
        assert np.array_equal(rgb[b], own_rgb), (name, b)
        if name in viz_cases.RESIZED:
            off = float(np.abs(res[b].astype(np.float64) - gold["disparity|%s|resized" % name][b]).max())
            print(name, b, "map off the fixture's by", off, "allowed", viz_ref.resample_tolerance(case["x"][b], h, w))
            assert off <= viz_ref.resample_tolerance(case["x"][b], h, w), (name, b)
            viz_ref.assert_resampled_close(rgb[b], rng[b], gold["disparity|%s|rgb" % name][b], gold["disparity|%s|range" % name][b], case["x"][b], magma)
        else:
            assert (rng[b, 0], rng[b, 1]) == tuple(gold["disparity|%s|range" % name][b]), (name, b)
            assert np.array_equal(rgb[b], gold["disparity|%s|rgb" % name][b]), (name, b)


def test_full_size_image(dev, gold):
    """375 x 1242, the case a double-precision percentile index misses; the fixture keeps the range and the SHA-256"""
    _, rgb, rng, _ = run(viz_cases.disparity("full"), dev)
    print("range", rng.tolist(), "fixture", gold["disparity|full|range"].tolist())
    assert np.array_equal(rng, gold["disparity|full|range"])
    assert hashlib.sha256(rgb.tobytes()).digest() == gold["disparity|full|sha256"].tobytes()


def test_poisoned_workspace_and_plain_outputs(dev, gold):
    """a second call on a workspace full of 0xFF gives the same bytes, with and without the optional outputs"""
    case = viz_cases.disparity("resize_12x40_47x155")
    x = torch.from_numpy(case["x"]).to(dev)
    first = viz.disparity_image(x, case["size"], case["q"])
    n = viz._lib.lib().wmd_viz_workspace_bytes(2, 47, 155)
    ws = torch.full(((n + 3) // 4,), -1, device=dev, dtype=torch.int32)
    again, rng = viz.disparity_image(x, case["size"], case["q"], return_range=True, workspace=ws)
    assert torch.equal(first, again)
    once_more = viz.disparity_image(x, case["size"], case["q"], workspace=ws)
    assert torch.equal(first, once_more)
    case = viz_cases.disparity("batch3")
    x = torch.from_numpy(case["x"]).to(dev)
    ws = torch.full((viz._lib.lib().wmd_viz_workspace_bytes(3, 9, 31) // 4 + 1,), -1, device=dev, dtype=torch.int32)
    assert np.array_equal(viz.disparity_image(x, workspace=ws).cpu().numpy(), gold["disparity|batch3|rgb"])


def test_input_forms_and_alignment(dev, gold):
    """[h,w] and [B,1,h,w] inputs; a picture whose bytes start off a dword boundary takes the byte-store path"""
    case = viz_cases.disparity("ragged_37x53")
    x = torch.from_numpy(case["x"]).to(dev)
    want = gold["disparity|ragged_37x53|rgb"]
    assert np.array_equal(viz.disparity_image(x[0]).cpu().numpy(), want)
    assert np.array_equal(viz.disparity_image(x[:, None]).cpu().numpy(), want)
    lib, buf = viz._lib.lib(), torch.zeros(37 * 53 * 3 + 8, device=dev, dtype=torch.uint8)
    ws = torch.empty(lib.wmd_viz_workspace_bytes(1, 37, 53) // 4 + 1, device=dev, dtype=torch.int32)
    for off in (1, 2, 3):
        viz.check(lib.wmd_viz_disparity(x.data_ptr(), 1, 37, 53, 37, 53, 95.0, viz.colormap("magma", dev).data_ptr(), buf.data_ptr() + off,
                                        None, None, ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream), "wmd_viz_disparity")
        assert np.array_equal(buf[off:off + 37 * 53 * 3].cpu().numpy().reshape(1, 37, 53, 3), want), off


def test_graph_capture_replays_to_the_same_bytes(dev, gold):
    case = viz_cases.disparity("resize_6x20_11x37")
    x = torch.from_numpy(case["x"]).to(dev)
    static = x.clone()
    eager = viz.disparity_image(static, case["size"], case["q"])          # also uploads the table outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = viz.disparity_image(static, case["size"], case["q"])
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(torch.flip(x, dims=(2,)))                                # another input through the same graph
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, viz.disparity_image(static, case["size"], case["q"]))


@pytest.mark.parametrize("name", viz_cases.COLORIZE)
@pytest.mark.parametrize("channels_first", (True, False))
def test_colorize_vs_fixture(dev, gold, name, channels_first):
    """the fixed 0.1 .. 10 range with values beyond both ends and a NaN; the automatic range; a constant plane under it.
    9 x 14 and 5 x 7 planes are no multiple of four pixels (byte stores when planar), the interleaved form packs"""
    case = viz_cases.colorize(name)
    out = viz.colorize(torch.from_numpy(case["x"]).to(dev), case["vmin"], case["vmax"], channels_first=channels_first)
    assert out.dtype == torch.uint8
    out = out.cpu().numpy()
    want = gold["colorize|" + name]
    assert np.array_equal(out if channels_first else out.transpose(0, 3, 1, 2), want)


def test_colorize_planar_packed_path(dev):
    """n a multiple of four: the planar output goes out as dwords"""
    case = viz_cases.colorize("fixed")
    x = np.ascontiguousarray(case["x"][:, :8, :12])
    out = viz.colorize(torch.from_numpy(x).to(dev), case["vmin"], case["vmax"]).cpu().numpy()
    plasma = viz_ref.table("plasma")
    want = np.stack([viz_ref.colorize(p, case["vmin"], case["vmax"], plasma).transpose(2, 0, 1) for p in x])
    assert np.array_equal(out, want)
    auto = viz.colorize(torch.from_numpy(x[:, :, :3]).to(dev).contiguous()[1], None, None).cpu().numpy()
    assert np.array_equal(auto, viz_ref.colorize(x[1, :, :3], None, None, plasma).transpose(2, 0, 1))


@pytest.mark.parametrize("name", viz_cases.NORMALIZE)
def test_normalize_image_vs_fixture(dev, gold, name):
    case = viz_cases.normalize(name)
    y = viz.normalize_image(torch.from_numpy(case["x"]).to(dev), per_image=case["per_image"]).cpu().numpy()
    assert y.shape == case["x"].shape
    assert np.array_equal(y.view(np.uint32), viz_ref.normalize_image(case["x"], case["per_image"]).view(np.uint32))
    assert np.array_equal(y.view(np.uint32), gold["normalize|" + name].view(np.uint32))
