"""GPU: the pose path (csrc/wmd_pose.hip, ops.transformation_from_parameters, ops.pose_head, kitti.PoseDecoder, kitti.PoseCNN,
photometric.predict_poses) against tests/pose_ref.py in float64 and against the reference's fixture.

Tensors that pass only through convolutions (axisangle, translation, feature and weight gradients) are held to the project's
1e-4 of the tensor's magnitude.  For T (rotation block and translation column apart, each relative to its own max |oracle64|),
the transform's gradients, and the end-to-end loss and pose-parameter gradients the tolerance is measured, not chosen
(the scheme of tests/test_gpu_photo_edges.py): on the same inputs
    e_ref = max |pose_ref32 - pose_ref64| / max |pose_ref64|        e_hip = max |hip - pose_ref64| / max |pose_ref64|
and the assertion is e_hip <= F[kind] * e_ref + 4 * 2^-23.  No case is excluded: the functions are smooth, and the one special
point, v = 0, is asserted exactly."""
import numpy as np
import pytest
import torch

from oracle import photo_ref as P
from wavelet_monodepth_amd import _lib, ops, synth
from wavelet_monodepth_amd import photometric as ph
import pose_cases as PC
import pose_ref as PR
import util as U

pytestmark = pytest.mark.gpu

RTOL = 1e-4
FLOOR = 4 * 2.0 ** -23
# per tensor kind, the smallest power of two >= twice the largest e_hip / e_ref measured on the MI355X among the comparisons whose
# e_hip exceeds the floor (where none does, among all of them: below the floor the bound holds whatever F is); the table is in
# DESIGN.md §4.6.  loss: the scalar losses; loss_dpose: the gradients of the total loss w.r.t. the pose network's parameters.
F = {"T_rot": 4, "T_trans": 4, "d_axisangle": 2, "d_translation": 4, "loss": 256, "loss_dpose": 8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def td(a, dev, g=False):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev).requires_grad_(g)


def tc(a, dtype, g=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(g)


def n64(v):
    return v.detach().cpu().double().numpy()


class Checks:
    """Prints e_ref, e_hip and the factor each comparison needs, then asserts all of them at once"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def add(self, kind, what, hip, o32, o64):
        hip, o32, o64 = (np.asarray(v, np.float64) for v in (hip, o32, o64))
        assert hip.shape == o64.shape, (what, hip.shape, o64.shape)
        e_ref, e_hip = U.edge_err(o32, o64), U.edge_err(hip, o64)
        print("POSE %-13s %-34s %-18s e_ref %.3e e_hip %.3e need_F %.2f" % (
            kind, self.case, what, e_ref, e_hip,
            max(e_hip - FLOOR, 0.0) / e_ref if e_ref > 0 else (0.0 if e_hip <= FLOOR else float("inf"))))
        if not e_hip <= F[kind] * e_ref + FLOOR:
            self.bad.append("%s %s: e_hip %.3e > %d * e_ref %.3e + %.1e" % (kind, what, e_hip, F[kind], e_ref, FLOOR))

    def add_T(self, what, hip, o32, o64):
        """[..., 4, 4]: the rotation block and the translation column apart; the bottom row is (0, 0, 0, 1) exactly"""
        self.add("T_rot", what + " R", hip[..., :3, :3], o32[..., :3, :3], o64[..., :3, :3])
        self.add("T_trans", what + " t", hip[..., :3, 3], o32[..., :3, 3], o64[..., :3, 3])
        assert np.array_equal(hip[..., 3, :], np.broadcast_to([0.0, 0.0, 0.0, 1.0], hip[..., 3, :].shape)), what

    def done(self):
        assert not self.bad, "%s: %s" % (self.case, "; ".join(self.bad))


# ---- the transform ----------------------------------------------------------------------------------------------------------

def ref_transform(v, t, g, invert, dtype):
    vv, tt = tc(v, dtype, True), tc(t, dtype, True)
    T = PR.transformation_from_parameters(vv[:, None], tt[:, None], invert)
    (T * tc(g, dtype)).sum().backward()
    return n64(T), n64(vv.grad), n64(tt.grad)


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "inverted"])
@pytest.mark.parametrize("N", [1, 65, 257])
def test_transform_vs_float64(dev, N, invert):
    """one lane, past a wave, past a block; angles 0, 1e-8, 1e-3, 0.1, 3.0 and pi in turn"""
    v, t, g = PC.transform_case(N)
    o64, o32 = ref_transform(v, t, g, invert, torch.float64), ref_transform(v, t, g, invert, torch.float32)
    vv, tt = td(v, dev, True), td(t, dev, True)
    T = ops.transformation_from_parameters(vv[:, None], tt[:, None], invert)
    assert T.shape == (N, 4, 4)
    (T * td(g, dev)).sum().backward()
    hip = n64(T), n64(vv.grad), n64(tt.grad)
    c = Checks("N=%d invert=%d" % (N, invert))
    c.add_T("T", hip[0], o32[0], o64[0])
    c.add("d_axisangle", "d_axisangle", hip[1], o32[1], o64[1])
    c.add("d_translation", "d_translation", hip[2], o32[2], o64[2])
    c.done()
    zero = ~v.any(1)
    assert zero.any()
    assert np.array_equal(hip[0][zero][:, :3, :3], np.broadcast_to(np.eye(3), (int(zero.sum()), 3, 3)))   # the identity, bit for bit
    for dv in (hip[1], o64[1], o32[1]):
        assert not dv[zero].any()                                                                          # as the reference gives
    assert np.array_equal(hip[2][zero], (-1.0 if invert else 1.0) * g[zero][:, :3, 3].astype(np.float64))


def test_transform_accepts_both_layouts_and_layers_exports(dev):
    from wavelet_monodepth_amd import layers
    v, t, _ = PC.transform_case(7)
    a = ops.transformation_from_parameters(td(v, dev), td(t, dev), True)
    b = layers.transformation_from_parameters(td(v, dev)[:, None], td(t, dev)[:, None], invert=True)
    assert torch.equal(a, b)
    rot, tra = layers.rot_from_axisangle(td(v, dev)[:, None]), layers.get_translation_matrix(td(t, dev))
    plain = ops.transformation_from_parameters(td(v, dev), td(t, dev))
    assert torch.equal(rot[:, :3, :3], plain[:, :3, :3]) and not rot[:, :3, 3].any()
    assert torch.equal(tra[:, :3, 3], plain[:, :3, 3]) and torch.equal(tra[:, :3, :3], torch.eye(3, device=dev).expand(7, 3, 3))


# ---- the pose head ------------------------------------------------------------------------------------------------------------

# (B, C, H, W, F): a single pixel; unaligned rows; 15 pixels; the training shape, more pixels than one pass of a wave; rows of
# 455 floats (unaligned, several passes); channels that are no multiple of 64
HEAD_SHAPES = [(1, 3, 1, 1, 1), (2, 8, 2, 2, 2), (2, 256, 3, 5, 1), (13, 256, 6, 20, 2), (2, 256, 7, 65, 2), (2, 70, 10, 32, 1)]
MODES = ("params", "T", "both")


def head_case(shape):
    B, C, H, W, Fr = shape
    bound = 1.0 / np.sqrt(C)
    return dict(x=synth.normal((B, C, H, W), "hd_x", 7), w=synth.uniform((6 * Fr, C, 1, 1), "hd_w", 7, -bound, bound),
                b=synth.uniform((6 * Fr,), "hd_b", 7, -bound, bound), ga=synth.uniform((B, Fr, 1, 3), "hd_ga", 7),
                gt=synth.uniform((B, Fr, 1, 3), "hd_gt", 7), gT=synth.uniform((B, Fr, 4, 4), "hd_gT", 7))


def head_loss(aa, tr, T, case, mode, conv):
    loss = 0
    if mode in ("params", "both"):
        loss = loss + (aa * conv(case["ga"])).sum() + (tr * conv(case["gt"])).sum()
    if mode in ("T", "both"):
        loss = loss + (T * conv(case["gT"])).sum()
    return loss


def ref_head(case, Fr, mask, scale, mode, dtype):
    x, w, b = (tc(case[k], dtype, True) for k in ("x", "w", "b"))
    aa, tr = PR.pose_tail(x, w, b, Fr, scale)
    T = torch.stack([PR.transformation_from_parameters(aa[:, f], tr[:, f], bool(mask >> f & 1)) for f in range(Fr)], 1)
    head_loss(aa, tr, T, case, mode, lambda a: tc(a, dtype)).backward()
    return [n64(v) for v in (aa, tr, T, x.grad, w.grad, b.grad)]


def hip_head(case, Fr, mask, scale, mode, dev):
    x, w, b = (td(case[k], dev, True) for k in ("x", "w", "b"))
    aa, tr, T = ops.pose_head(x, w, b, Fr, invert_mask=mask, scale=scale)
    head_loss(aa, tr, T, case, mode, lambda a: td(a, dev)).backward()
    return [aa, tr, T, x.grad, w.grad, b.grad]


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pose_head_vs_float64(dev, shape):
    """every invert mask, backward from d_params alone, from dT alone and from both; mask 3 runs with scale = 1 (angles of the
    order of 0.1 instead of 0.001)"""
    B, C, H, W, Fr = shape
    case = head_case(shape)
    c = Checks("x".join(map(str, shape)))
    for mask in range(4):
        scale = 1.0 if mask == 3 else 0.01
        for mode in MODES:
            o64, o32 = ref_head(case, Fr, mask, scale, mode, torch.float64), ref_head(case, Fr, mask, scale, mode, torch.float32)
            got = hip_head(case, Fr, mask, scale, mode, dev)
            what = "mask %d %s" % (mask, mode)
            assert got[0].shape == (B, Fr, 1, 3) and got[1].shape == (B, Fr, 1, 3) and got[2].shape == (B, Fr, 4, 4)
            hip = [n64(v) for v in got]
            for k, name in ((0, "axisangle"), (1, "translation"), (3, "dx"), (4, "dw"), (5, "dbias")):
                U.assert_close(hip[k], o64[k], RTOL, "%s %s %s" % (c.case, what, name))
            c.add_T(what, hip[2], o32[2], o64[2])
    c.done()


def test_pose_head_backward_is_reproducible(dev):
    """the sums over B run in a fixed order: two runs of the B = 13 case give the same bits"""
    case = head_case(HEAD_SHAPES[3])
    a, b = hip_head(case, 2, 1, 0.01, "both", dev), hip_head(case, 2, 1, 0.01, "both", dev)
    for u, v, name in zip(a, b, ("axisangle", "translation", "T", "dx", "dw", "dbias")):
        assert torch.equal(u, v), name


def test_pose_head_launch_count(dev):
    """one library kernel forward, at most two backward"""
    case = head_case(HEAD_SHAPES[3])
    x, w, b = (td(case[k], dev, True) for k in ("x", "w", "b"))
    _lib.profile_begin()
    aa, tr, T = ops.pose_head(x, w, b, 2, invert_mask=1)
    recs = _lib.profile_end()
    assert [(r["kernel"], r["calls"]) for r in recs] == [("pose_head_fwd_kernel", 1)], recs
    loss = head_loss(aa, tr, T, case, "both", lambda a: td(a, dev))
    _lib.profile_begin()
    loss.backward()
    recs = _lib.profile_end()
    assert 1 <= sum(r["calls"] for r in recs) <= 2 and all(r["kernel"].startswith("pose_head_bwd") for r in recs), recs
    assert x.grad is not None and w.grad is not None and b.grad is not None


# ---- the networks -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return U.load_golden("kitti_pose.npz")


@pytest.mark.parametrize("name", list(PC.NETS))
def test_networks_vs_reference_and_float64(dev, gold, name):
    """PoseDecoder on the last map of a 64x64 frame (2x2) with two features, with one feature and two frames, and at 6x20;
    PoseCNN(2) on 64x64 images: outputs, the gradient of every input and of every parameter, against the reference's own
    float64 run (the fixture, sampled) and against pose_ref in float64 (every entry)"""
    kind, kw, _ = PC.NETS[name]
    module = synth.fill_state_dict(PC.build(kind, kw), seed=PC.SEED)
    o64 = PC.run_net(PC.RefModule(module, kind, PC.frames_of(name), torch.float64), name, torch.float64)
    got = PC.run_net(module.to(dev), name, torch.float32, dev)
    assert set(got) == set(o64) and {"d" + k for k in module.state_dict()} <= set(got)
    for k, v in got.items():
        U.assert_close(v, o64[k], RTOL, "%s %s vs pose_ref64" % (name, k))
        fix = gold["%s|f64|%s" % (name, k)]
        U.assert_close(v if k in ("axisangle", "translation") else U.sample(v, PC.SAMPLE), fix, RTOL, "%s %s vs the reference" % (name, k))


def test_pose_decoder_three_features(dev):
    """three or more features: the remainder is concatenated before ("pose", 0)"""
    kw = dict(num_ch_enc=[16, 16, 24, 32, 40], num_input_features=3)
    module = synth.fill_state_dict(PC.build("decoder", kw), seed=5)
    xs = [np.maximum(synth.normal((2, 40, 3, 5), "p3_in%d" % i, 5), 0.0) for i in range(3)]
    sd = {k: v.double() for k, v in module.state_dict().items()}
    want = PR.pose_decoder([[tc(x, torch.float64)] for x in xs], sd, 2)
    module = module.to(dev)
    with torch.no_grad():
        got = module([[td(x, dev)] for x in xs])
    for g, w_, nm in zip(got, want, ("axisangle", "translation")):
        assert g.shape == (2, 2, 1, 3)
        U.assert_close(g, w_, RTOL, nm)


# ---- end to end: features -> poses -> warps -> loss ------------------------------------------------------------------------------

def e2e_run(kind, module, inp, out, feats, opt, where, dtype):
    """-> (losses, {parameter name: gradient}) on the GPU (where = a device) or in the oracle (where = None)"""
    hip = where is not None
    conv = (lambda a: torch.from_numpy(a).to(where)) if hip else (lambda a: torch.from_numpy(a).to(dtype))
    i2, o2 = {k: conv(v) for k, v in inp.items()}, {k: conv(v) for k, v in out.items()}
    f2 = {f: [conv(a) for a in fl] for f, fl in feats.items()}
    if hip:
        module.zero_grad(set_to_none=True)
        o2.update(ph.predict_poses(i2, f2, {"pose": module}, opt))
        ph.generate_images_pred(i2, o2, opt)
        losses = ph.compute_losses(i2, o2, opt, tie_break_noise=0.0)
        losses["loss"].backward()
        return losses, {k: p.grad for k, p in module.named_parameters()}
    ref = PC.RefModule(module, "cnn" if kind == "posecnn" else "decoder", 1, dtype)
    o2.update(PR.predict_poses(i2, f2, {"pose": ref}, opt))
    (PR.generate_images_pred_posecnn if kind == "posecnn" else P.generate_images_pred)(i2, o2, opt)
    losses = P.compute_losses(i2, o2, opt)
    losses["loss"].backward()
    return losses, {k: p.grad for k, p in ref.named_parameters()}


@pytest.mark.parametrize("kind", ["shared", "posecnn"])
def test_poses_to_loss_vs_float64(dev, kind):
    """predict_poses -> generate_images_pred -> compute_losses on loss_case() at 32x64: the warp's dT and the pose chain in one
    graph.  "shared": PoseDecoder on random ResNet18 features of the three frames (pairs in temporal order, f = -1 inverted);
    "posecnn": PoseCNN on the image pairs, the transform rebuilt per scale from the mean inverse depth."""
    inp, out = U.loss_case()
    out = {k: v for k, v in out.items() if k[0] != "cam_T_cam"}
    feats = {}
    if kind == "shared":
        feats = {f: [np.maximum(a, 0.0) for a in synth.encoder_features(2, 32, 64, U.R18, seed=40 + f)] for f in (0, -1, 1)}
        module = PC.build("decoder", dict(num_ch_enc=U.R18, num_input_features=2))
    else:
        for f in (0, -1, 1):
            inp[("color_aug", f, 0)] = inp[("color", f, 0)]
        module = PC.build("cnn", dict(num_input_frames=2))
    module = synth.fill_state_dict(module, seed=11)
    opt = ph.LossOptions(height=32, width=64, pose_model_type=kind, pose_model_input="pairs")
    l64, g64 = e2e_run(kind, module, inp, out, feats, opt, None, torch.float64)
    l32, g32 = e2e_run(kind, module, inp, out, feats, opt, None, torch.float32)
    lg, gg = e2e_run(kind, module.to(dev), inp, out, feats, opt, dev, torch.float32)
    assert set(lg) == set(l64) and set(gg) == set(g64)
    c = Checks(kind)
    for k in l64:
        c.add("loss", k, *(float(l[k].detach()) for l in (lg, l32, l64)))
    for k in g64:
        assert float(g64[k].abs().max()) > 0, k
        c.add("loss_dpose", "d" + k, n64(gg[k]), n64(g32[k]), n64(g64[k]))
    c.done()


def test_predict_poses_all_frames_mode(dev):
    """pose_model_input = "all" with the shared encoder: one pass over the three feature lists, two predicted frames, frame f's
    transform is prediction number i and is never inverted; the "s" frame is skipped"""
    feats = {f: [np.maximum(a, 0.0) for a in synth.encoder_features(2, 32, 64, U.R18, seed=40 + f)] for f in (0, -1, 1)}
    module = synth.fill_state_dict(PC.build("decoder", dict(num_ch_enc=U.R18, num_input_features=3)), seed=11)
    opt = ph.LossOptions(height=32, width=64, frame_ids=(0, -1, 1, "s"), pose_model_type="shared", pose_model_input="all")
    want, want32 = (PR.predict_poses({}, {f: [tc(a, dt) for a in fl] for f, fl in feats.items()},
                                     {"pose": PC.RefModule(module, "decoder", 2, dt)}, opt) for dt in (torch.float64, torch.float32))
    module = module.to(dev)
    with torch.no_grad():
        got = ph.predict_poses({}, {f: [td(a, dev) for a in fl] for f, fl in feats.items()}, {"pose": module}, opt)
    assert set(got) == set(want) == {(n, 0, f) for n in ("axisangle", "translation", "cam_T_cam") for f in (-1, 1)}
    c = Checks("all frames")
    for k in want:
        if k[0] == "cam_T_cam":
            c.add_T(U.key_str(k), n64(got[k]), n64(want32[k]), n64(want[k]))
        else:
            U.assert_close(got[k], want[k], RTOL, U.key_str(k))
    c.done()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------

def test_pose_decoder_forward_backward_in_one_graph(dev):
    """forward_transforms + backward captured on a single stream: nothing synchronises the host or allocates outside the
    torch allocator, and two replays give the eager result bit for bit"""
    name = "dec_r18_6x20"
    kind, kw, _ = PC.NETS[name]
    module = synth.fill_state_dict(PC.build(kind, kw), seed=PC.SEED).to(dev)
    xs = [td(a, dev, True) for a in PC.net_inputs(name)]
    ga, gt = (td(g, dev) for g in PC.out_weights(name))
    gT = td(synth.uniform((2, 1, 4, 4), "graph_gT", 3), dev)
    leaves = xs + list(module.parameters())

    def step():
        aa, tr, T = module.forward_transforms([[x] for x in xs], invert_mask=1)
        loss = (aa * ga).sum() + (tr * gt).sum() + (T * gT).sum()
        return [aa, tr, T] + list(torch.autograd.grad(loss, leaves))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                           # tile choices and weight images are made outside the capture
        eager = [v.detach().clone() for v in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for v in outs:
            v.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, (u, v) in enumerate(zip(outs, eager)):
            assert torch.equal(u.detach(), v), "output %d of the replay differs from the eager run" % k
