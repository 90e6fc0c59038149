"""SparseDepthWaveProgressiveDecoder on MI355X — API-compatible with the reference class
(KITTI/networks/decoders/depth_decoder.py:171-428): same constructor, parameters and
state_dict keys as the dense decoder (checkpoints are interchangeable), `forward(input_features,
thresh_ratio=0.05, sparse_scales=[0,1,2,3])`, same output keys incl. the five mask families and the
`total_ops` op model.  Inference only; batch 1 like the reference, or (extension) a batch of frames decoded together.

The five masks of the coarsest level (always all ones) are views of one cached constant shared by every call: treat the returned
masks as read-only.

Differences that are not observable in the outputs: activations stay dense and zero-initialised instead of
being compacted (see include/wmd.h); the forward never waits for the GPU -- the python-int `total_ops` entries are
resolved from the device-side pixel counts on first access (sparse_ops.LazyOpsDict), so independent frames can be
decoded concurrently on several streams; nothing is printed (the reference prints 'sparse: i').
`sparse_scales`: a level outside the list runs densely.  The reference only survives lists whose sparse levels are the
finest ones (its dense branch keeps reading the stale dense activation of the last dense level and crashes on the channel
mismatch); here a dense level below a sparse one simply convolves the zero-initialised sparse activations.
"""
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops, sparse_ops as S
from ..wavelets import IDWT
from ..graphs import GraphCache
from .depth_decoder import _build_wave_convs
from ..layers import split_edge


def _conv_ops(cin, cout, npix, k):
    # dense layers: (1 + k*k*cin*npix) * cout — the "1 +" sits inside the pixel product (reference :386-398)
    return (1 + k * k * cin * npix) * cout


def _round64(n):
    return (int(n) + 63) // 64 * 64


def _sparse_conv_ops(cin, cout, nnz_out, mid=None):
    ops_ = 0
    if mid is not None:                       # fused leading 1x1 (layers.py:405)
        cin_mid, cmid, nnz_in = mid
        ops_ += nnz_in * cin_mid * cmid + nnz_in * cmid
    ops_ += cin * 9 * nnz_out                 # gathered elements (layers.py:462)
    ops_ += (1 + 9 * cin) * nnz_out * cout    # layers.py:469
    return ops_


def level_static_ops(i, h, w, sparse, trunk=None, heads=()):
    """Pixel-count independent part of the reference's op model for decoder level i working on an h x w coarse grid
    (depth_decoder.py:296-417): threshold + dilation arithmetic, the four mask2idxmap calls of a sparse level or the
    dense layers of a dense one, and the IDWT.  trunk = ((Cin0, Cout0), (Cin1, Cout1)), heads = [(Cin, Cmid, Cin3,
    Cout3), ...] are only read for a dense level."""
    H2, W2 = 2 * h, 2 * w
    n = 0
    if i != 4:
        n += 3 * h * w                                # max |yh| over three bands + compare (:308-309)
    n += 25 * h * w + 100 * h * w                     # MaxPool 5x5 on the coarse grid, 5x5 on the fine grid (:313-319)
    if sparse:
        n += 2 * h * w + 2 * H2 * W2                  # four mask2idxmap calls (layers.py:388)
    else:
        (ci0, co0), (ci1, co1) = trunk
        n += _conv_ops(ci0, co0, h * w, 3) + _conv_ops(ci1, co1, H2 * W2, 3)
        for cin, cmid, cin3, cout3 in heads:
            n += _conv_ops(cin, cmid, H2 * W2, 1) + _conv_ops(cin3, cout3, H2 * W2, 3)
    n += 4 * (2 * H2) * (2 * W2)                      # IDWT output pixels x 4 (:373,417)
    return n


def resolve_total_ops(static_ops, counters, counts):
    """The reference's per-scale and total op counts from the static parts, the layer widths of every sparse level
    (counters: (level, _, (Cin0, Cout0), (Cin1, Cout1), (Cin_1x1, Cmid), (Cin3, Cout3))) and that level's pixel
    counts (counts[level] = (upconv0, upconv1, wavelet) mask sums).  -> ({scale: ops}, total)."""
    per_scale, total = {}, 0
    for i in sorted(static_ops, reverse=True):
        n = static_ops[i]
        for (lvl, _nnz, (ci0, co0_), (ci1, co1_), (cim, cm), (ci3, co3)) in counters:
            if lvl != i:
                continue
            n0, n1, nw = counts[lvl]
            n += _sparse_conv_ops(ci0, co0_, n0) + _sparse_conv_ops(ci1, co1_, n1)
            n += 2 * _sparse_conv_ops(ci3, co3, nw, mid=(cim, cm, n1))
        per_scale[i - 1] = n
        total += n
    return per_scale, total


SPECS = [(1, 1), (1, 2), (2, 2), (2, 1), (2, 0)]   # lowres, upconv0, upsample, upconv1, wavelet (:311-319)

SparseSwitches = namedtuple("SparseSwitches", "tiles lists tile big_from list_from unfused_masks")


def sparse_switches():
    """Every WMD_SPARSE_* switch of this decoder, read once per forward (tests change them between forwards of one process).
    tiles / lists choose the form of the sparse levels (_device_chain, _lists_ok), tile / big_from / list_from the shape of a
    work-list launch (_list_tile); unfused_masks: the three-launch mask form of one frame without a LevelState."""
    env = os.environ.get
    return SparseSwitches(tiles=env("WMD_SPARSE_TILES", "1") != "0", lists=env("WMD_SPARSE_LISTS", "1") != "0",
                          tile=env("WMD_SPARSE_TILE"), big_from=int(env("WMD_SPARSE_BIG_FROM", "700")),
                          list_from=int(env("WMD_SPARSE_LIST_FROM", "800")),
                          unfused_masks=env("WMD_SPARSE_UNFUSED_MASKS", "0") == "1")


def _sparse_levels(sparse_scales):
    """The levels that can run sparsely, coarse to fine (level 4 has no low-pass plane to threshold, 0 is ignored)."""
    return [i for i in (3, 2, 1) if i in sparse_scales]


def _list_tile(sw, B, hh, ww, cout, cin=8, c_up=8):
    """Tile shape of a work-list launch, or None: the launch takes the mask form of the same level."""
    # 8x16 (128-pixel workgroups: the finest granularity, most parallelism for one frame)
    # until the launch could hold more than WMD_SPARSE_BIG_FROM (item = tile x 32-channel slab) of them, 16x16 beyond (a batch
    # of frames: at full density the 8x16 form costs 35 % more than 256-pixel workgroups, while on contour masks both skip
    # about the same share of the work); WMD_SPARSE_TILE=HxW forces one shape.
    # ... and no list at all below WMD_SPARSE_LIST_FROM items (one frame; the coarse launches of a batch): the launch then runs the masked kernel the autotuner
    # picked for the shape (a block per tile tests its own mask bytes; host-chosen split-K) -- with a few dozen tiles on 256 CUs
    # nothing is gained by compacting them, and the tuned 16x16x4 / 32x32x2 kernels of round 3 are 10-20 % faster per launch
    # than the list kernel's one tile shape (r04_sparse_timelines.txt: 99 + 25 us of convolutions + reduces against 107 + 37)
    # (threshold swept at 12 frames, contour masks 0.10 / 0.03 / 0.01: 256 -> 0.633 ms, 500 -> 0.605, 800 -> 0.585, 1500 -> 0.630,
    #  no lists -> 0.689; dense 0.644-0.666: the lists pay on the two large launches of a batch -- upconv(2,1), upconv(1,1) --
    #  where tail rounds of whole tiles are what skipping loses, and cost on the small ones)
    # a LIST launch needs the flattened staging (wino32_pure: every 8-channel chunk inside one source tensor) and a tile
    # shape the library has a work-list kernel for; anything else takes the mask form of the same level
    if cin % 8 or c_up % 8:
        return None
    if sw.tile:
        th, tw = (int(v) for v in sw.tile.split("x"))
        return (th, tw) if _lib.lib().wmd_conv_list_tile_supported(th, tw) else None
    items = B * (-(-hh // 8)) * (-(-ww // 16)) * (-(-cout // 32))
    if items < sw.list_from:
        return None
    return (16, 16) if items > sw.big_from else (8, 16)


class _Planes:
    """Activation planes handed out of one flat float buffer, in order; every plane set starts 256-byte aligned."""

    def __init__(self, buf):
        self.buf, self.used = buf, 0

    def take(self, *shape):
        n = int(np.prod(shape))
        v = self.buf[self.used:self.used + n].view(*shape)
        self.used += _round64(n)
        return v


def _fused_heads(sw, width):
    """A sparse level of this width runs its heads on the dense fused head kernels (block-sparse forms, supported width)."""
    return sw.tiles and int(width) in ops.FUSED_HEAD_WIDTHS


def _unpack(m):
    return m[0].conv.weight, m[0].conv.bias, m[2].conv.weight, m[2].conv.bias


def _store_level(out, i, B, masks, yl, yh, disp):
    for name, m in zip(("lowres_mask", "upconv0_mask", "upsample_mask", "upconv1_mask", "wavelet_mask"), masks):
        out[(name, i - 1)] = m.view(torch.bool).reshape(B, 1, *m.shape[-2:])
    out[("wavelets", i - 1, "LL")] = yl
    out[("wavelets", i - 1, "LH")] = yh[:, :, 0]
    out[("wavelets", i - 1, "HL")] = yh[:, :, 1]
    out[("wavelets", i - 1, "HH")] = yh[:, :, 2]
    out[("disp", i - 1)] = disp


class SparseDepthWaveProgressiveDecoder(nn.Module):
    def __init__(self, num_ch_enc, scales=range(4), num_output_channels=1, use_skips=True):
        super().__init__()
        self.num_output_channels = num_output_channels
        self.use_skips = use_skips
        self.upsample_mode = "nearest"
        self.scales = scales
        self.num_ch_enc = num_ch_enc
        self.num_ch_dec = np.array([16, 32, 64, 128, 256])
        self.J = 1
        self.inverse_wt = IDWT(wave="haar", mode="zero")
        self.convs = _build_wave_convs(self.num_ch_enc, self.num_ch_dec, use_skips)
        self.decoder = nn.ModuleList(list(self.convs.values()))
        self.sigmoid = nn.Sigmoid()
        self._graph_mode = False
        self._graphs = GraphCache()
        self._edge = None
        self._side = None          # stream of the activation-pool fill
        self._ones = {}            # all-ones mask constants of the coarsest level, per (device, B, h, w)
        self._states = {}          # sparse_ops.LevelState of the work-list form, per input signature

    # ------------------------------------------------------------------------------------------
    def _dense_coefficients(self, x, i, with_ll):
        heads = ([0] if with_ll else []) + [1, -1]
        mods = [self.convs[("waveconv", i, j)] for j in heads]
        mid = ops.conv1x1_stacked_nograd(x, [m[0].conv.weight for m in mods], [m[0].conv.bias for m in mods],
                                         act="leaky", slope=0.1)
        offs, o = {}, 0
        for j, m in zip(heads, mods):
            offs[j] = o
            o += m[0].conv.weight.shape[0]
        yl = None
        if with_ll:
            c3 = mods[0][2].conv
            yl = ops.head3x3_nograd(mid, c3.weight.shape[1], offs[0], c3.weight, c3.bias, pad="reflect", mode=1,
                                    scale=2.0 ** i)
        cp, cn = self.convs[("waveconv", i, 1)][2].conv, self.convs[("waveconv", i, -1)][2].conv
        yh = ops.head3x3_nograd(mid, cp.weight.shape[1], offs[1], cp.weight, cp.bias, offs[-1], cn.weight, cn.bias,
                                pad="reflect", mode=2, scale=2.0 ** (i - 1))
        return yl, yh.unsqueeze(1)

    def enable_graph(self, on=True):
        """Capture the whole device-side chain (≈35 launches, all pixel counts stay on the device) into one hipGraph
        per (inputs, threshold, scales) and replay it; only the python-int op model is computed on the host after."""
        self._graph_mode = bool(on)
        self._graphs.clear()
        self._states.clear()
        self._ones.clear()
        return self

    @torch.no_grad()
    def forward(self, input_features, thresh_ratio=0.05, sparse_scales=[0, 1, 2, 3], _force_masks=None):
        # The reference asserts batch 1 ("works with single input only", depth_decoder.py:297).  Extension: a batch decodes
        # B frames -- each with its own coefficient range, masks, pixel lists and counts -- through the SAME launches (one
        # 640x192 frame is a few dozen to a few hundred 16-pixel tiles per launch and cannot fill 256 CUs); every per-frame
        # output equals the batch-1 result, and the `total_ops` entries become lists with one integer per frame.
        input_features, edge = split_edge(input_features)       # encoder edge: the last feature may be a pre-activation
        self._edge = edge
        S._on_gpu(*input_features)      # fails loudly on CPU tensors: there is no fallback path
        forced_on_device = _force_masks is None or all(m.is_cuda for m in _force_masks.values())
        graph = self._graph_mode and forced_on_device
        sw = sparse_switches()
        state = self._level_state(input_features, sparse_scales, _force_masks, graph, sw)
        if state is not None:
            state.before_forward()
        if graph:
            thr, scales = float(thresh_ratio), tuple(sparse_scales)
            lv = sorted(_force_masks) if _force_masks else []      # injected masks are live inputs of the graph too
            nf = len(input_features)
            res = self._graphs.run(lambda f: self._device_chain(f[:nf], thr, scales, dict(zip(lv, f[nf:])) if lv else None, state, sw),
                                   list(input_features) + [_force_masks[i] for i in lv], self.parameters(),
                                   extra_key=(thr, scales, tuple(lv), state is not None) + (("edge",) + edge.key() if edge is not None else ()))
            out, counters, static_ops = dict(res[0]), res[1], res[2]
            if state is not None:
                state.seq += 1          # the replay (the warm-up executions of a capture counted themselves)
        else:
            out, counters, static_ops = self._device_chain(input_features, thresh_ratio, sparse_scales, _force_masks, state, sw)
        res = self._host_op_model(out, counters, static_ops, state)
        self.outputs = res      # depth_decoder.py:293,379,423,427: the op counts live in self.outputs too
        return res

    # ------------------------------------------------------------------------------------------
    def _pool_floats(self, input_features, lv, B, sw):
        """Floats of the activation planes of the sparse levels lv: the outputs of upconv(i,0) and upconv(i,1), plus the stacked
        mid channels and yh of a level whose heads run as gather-GEMMs; every plane 64-float aligned."""
        n = 0
        for i in lv:
            hh, ww = input_features[i].shape[-2:]
            c0, c1 = (self.convs[("upconv", i, j)].conv.conv.weight.shape[0] for j in (0, 1))
            n += _round64(B * c0 * hh * ww) + _round64(B * c1 * 4 * hh * ww)
            if not _fused_heads(sw, c1):
                cm = self.convs[("waveconv", i, 1)][0].conv.weight.shape[0]
                n += _round64(B * 2 * cm * 4 * hh * ww) + _round64(B * 3 * 4 * hh * ww)
        return n

    def _lists_ok(self, sparse_scales, _force_masks, sw):
        """The work-list form (default) serves the tile form when the sparse levels are the finest ones (a dense level BELOW a
        sparse one would read the never-refilled activation pool), every sparse level's heads run on the fused kernels and
        level 4 is not injected.  WMD_SPARSE_LISTS=0: the round-3 tile form (pool fill + per-block mask tests + count copy)."""
        if not (sw.lists and sw.tiles and self.use_skips):
            return False
        if _force_masks is not None and 4 in _force_masks:
            return False
        if any(i > 3 for i in set(sparse_scales)):
            # level 4 has no low-pass plane to threshold: the reference and the tile form fail an assertion there -- so must this
            # form (it used to drop the level silently and run it densely); 0 is ignored by every form
            return False
        lv = _sparse_levels(sparse_scales)
        if not lv or lv != list(range(lv[0], 0, -1)):
            return False
        widths = [int(self.convs[("upconv", i, 1)].conv.conv.weight.shape[0]) for i in lv]
        return all(wd in ops.FUSED_HEAD_WIDTHS and wd % 8 == 0 for wd in widths) and int(self.num_ch_dec[4]) in ops.FUSED_HEAD_WIDTHS

    def _level_state(self, input_features, sparse_scales, _force_masks, graph, sw):
        """The persistent device state of the work-list form for this input signature (None: another form runs).  In graph
        mode one state per captured graph (keyed like the graph: the captured launches hold its pointers; kept alive by the
        graph entry), else one per (stream, shapes)."""
        if not self._lists_ok(sparse_scales, _force_masks, sw):
            return None
        x = input_features[-1]
        B, dev = x.shape[0], x.device
        lv = _sparse_levels(sparse_scales)
        shapes = tuple(tuple(f.shape) for f in input_features)
        if graph:
            key = ("g", dev.index, tuple(f.data_ptr() for f in input_features), shapes, tuple(lv[::-1]))
        else:
            key = ("e", dev.index, torch.cuda.current_stream(dev).cuda_stream, shapes, tuple(lv[::-1]))
        st = self._states.get(key)
        if st is None:
            if len(self._states) >= 64:
                self._states.clear()
                self._graphs.clear()       # captured launches hold the states' pointers
            st = S.LevelState(dev, B, len(lv), self._pool_floats(input_features, lv, B, sw))
            self._states[key] = st
        return st

    def _forward_pool(self, dev, B, plane_floats, n_sparse):
        """The per-forward activation pool of the forms without a LevelState -> (planes, the [n_sparse,B,3] pixel counts in its
        tail, join: to be called before the first sparse level takes its first plane)."""
        # every zero-initialised activation plane of the sparse levels comes out of ONE pooled buffer (one fill per
        # forward instead of four per level; at batch 1 the chain is launch-latency bound)
        if not n_sparse:
            return None, None, lambda: None
        nnz_off = plane_floats
        pool_floats = plane_floats + _round64(n_sparse * B * 3)       # the pixel counts of every sparse level share the fill (int32 zeros)
        # ... filled on a side stream while the dense coarsest level runs when it is large (41 us at batch 12; at batch 1 the
        # fill takes 9 us and so does the stream join); joined before the first sparse level takes its first plane
        fill_stream = [None]
        pool = torch.empty(pool_floats, device=dev)
        cur = torch.cuda.current_stream(dev)
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        if pool_floats * 4 >= (16 << 20):
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                pool.zero_()
            if not torch.cuda.is_current_stream_capturing():
                pool.record_stream(self._side)
            fill_stream[0] = self._side
        else:                      # one frame: the join of a second stream costs as much as the fill itself
            pool.zero_()

        def join_fill():
            if fill_stream[0] is not None:
                torch.cuda.current_stream(dev).wait_stream(fill_stream[0])
                fill_stream[0] = None

        all_nnz = pool[nnz_off:nnz_off + n_sparse * B * 3].view(torch.int32).view(n_sparse, B, 3)
        return _Planes(pool), all_nnz, join_fill

    def _device_chain(self, input_features, thresh_ratio, sparse_scales, _force_masks, state=None, sw=None):
        """The level loop of every form: per level its masks -> the sparse or the dense level -> the ten outputs -> the Haar
        synthesis where the head kernels did not run it.  The three forms of a sparse level are choices inside those steps.
        Default: block-sparse execution of the dense Winograd kernels over the pixel TILES that hold active pixels + the dense
        fused head kernels with the wavelet mask in their epilogue (batch 1: 0.30 ms against 0.33 ms, batch 12 at 10 % density:
        0.75 ms against 1.18 ms); with a LevelState (see _lists_ok) in its work-list form (round 4) -- per level ONE mask launch
        (threshold from the range keys the previous level's head epilogue left behind, the five masks, the active-tile lists of
        both trunk convolutions, the pixel counts into the ring) -> upconv(i,0) and upconv(i,1) over the listed tiles only, K
        split chosen on the device -> the fused head kernels, skipping pixel runs / wavefronts without an active pixel; no pool
        fill, no count copy.  WMD_SPARSE_TILES=0: gather-GEMMs over compacted pixel lists, the literal form of
        KITTI/layers.py:337-507."""
        sw = sw or sparse_switches()
        S._on_gpu(*input_features)      # fails loudly on CPU tensors: there is no fallback path
        x = input_features[-1].contiguous()
        B, dev = x.shape[0], x.device    # frames decoded together: every frame has its own range, masks, pixel lists and counts
        lv = _sparse_levels(sparse_scales)
        c = SimpleNamespace(sw=sw, state=state, feats=input_features, B=B, dev=dev, thresh=thresh_ratio, force=_force_masks, lv=lv,
                            counters=[],            # (level, nnz tensor [B,3] or None, layer widths) resolved into python ints lazily
                            static_ops={},
                            keys_armed=False,       # the head of the level above folded its LL range into state.keys
                            prev_upconv1=None)      # upconv1 mask of the sparse level above (= the support of the activations this level reads)
        if state is not None:
            capturing = torch.cuda.is_current_stream_capturing()
            c.planes, c.all_nnz, join_fill = _Planes(state.pool), None, None
        else:
            c.planes, c.all_nnz, join_fill = self._forward_pool(dev, B, self._pool_floats(input_features, lv, B, sw), len(lv))
        scales = set(sparse_scales)
        out = {}
        yl = yh = None
        src = x                # dense [B,C,h,w] activations carried between levels
        for i in range(4, 0, -1):
            h, w = src.shape[-2:]
            c0, c1 = self.convs[("upconv", i, 0)].conv.conv, self.convs[("upconv", i, 1)].conv.conv
            forced = _force_masks is not None and i in _force_masks
            sparse = i in scales
            if sparse and state is None:
                join_fill()         # the counts and every activation plane of the sparse levels live in the pool
            masks, lists, lowres_in, counted = self._level_masks(c, i, h, w, c0, c1, yl, yh, sparse, forced)
            want_keys = state is not None and (i - 1) in lv and not (_force_masks is not None and (i - 1) in _force_masks)
            if sparse:
                src, yh, synthesis = self._sparse_level(c, i, c0, c1, src, yl, masks, lists, lowres_in, counted, want_keys)
                if state is not None:
                    c.prev_upconv1 = masks[3]
            else:
                # the work-list form completes every dense level on the fused head kernels (a select on the wavelet mask); the
                # other forms only the dense level of every decode, and multiply by the mask below it
                fused = state is not None or (i == 4 and not forced and int(c1.weight.shape[0]) in ops.FUSED_HEAD_WIDTHS)
                src, yl, yh, synthesis = self._dense_level(c, i, c0, c1, src, yl, masks[4], fused, want_keys)
            yl_next, disp = synthesis or ops.idwt_haar(yl, yh, disp_scale=1.0 / 2 ** (i - 1), clamp01=True)
            _store_level(out, i, B, masks, yl, yh, disp)
            yl = yl_next
        if state is not None and not capturing:
            state.seq += 1      # an eager execution advanced the device's forward counter (a capture executes nothing)
        return out, c.counters, c.static_ops

    # ------------------------------------------------------------------------------------------
    def _ones_masks(self, dev, B, h, w):
        # all-ones mask: every dilation of it is all ones too (MaxPool2d pads with -inf) -- one constant, five views
        ones = self._ones.get((dev, B, h, w))
        if ones is None:
            ones = self._ones[(dev, B, h, w)] = torch.ones(B * (2 * h * w + 3 * 4 * h * w), device=dev, dtype=torch.uint8)
        o4 = 2 * B * h * w
        return [ones[:B * h * w].view(B, h, w), ones[B * h * w:o4].view(B, h, w)] + \
               [ones[o4 + k * 4 * B * h * w:o4 + (k + 1) * 4 * B * h * w].view(B, 2 * h, 2 * w) for k in range(3)]

    @staticmethod
    def _base_mask(_force_masks, i, B, h, w, dev):
        mask = _force_masks[i].to(dev).reshape(-1, h, w).to(torch.uint8)
        if mask.shape[0] != B:           # one injected mask shared by every frame
            mask = mask.expand(B, h, w)
        return mask

    def _level_masks(self, c, i, h, w, c0, c1, yl, yh, sparse, forced):
        """-> (the five masks of SPECS, the tile lists of a work-list level or None, the input support of upconv(i,0), the counts
        the mask launch accumulated itself or None)."""
        B, state = c.B, c.state
        if sparse and state is not None:
            k = len(c.counters)
            (C0, cin0), (C1_, cin1) = c0.weight.shape[:2], c1.weight.shape[:2]
            skip_c = c.feats[i - 1].shape[1]
            specs = [SPECS[0] + (0, None), SPECS[1] + (1, _list_tile(c.sw, B, h, w, C0, cin0)), SPECS[2] + (0, None),
                     SPECS[3] + (2, _list_tile(c.sw, B, 2 * h, 2 * w, C1_, cin1, C0 if skip_c else 8)), SPECS[4] + (3, None)]
            if c.prev_upconv1 is not None:     # input support of upconv(i,0): lowres AND the previous sparse level's support
                specs.append(SPECS[0] + (0, None, c.prev_upconv1))
            source = dict(mask0=self._base_mask(c.force, i, B, h, w, c.dev)) if forced else dict(thresh_ratio=c.thresh, yl=yl, yh=yh)
            masks, lists = S.mask_level_lists(state, B, h, w, specs, use_keys=c.keys_armed, counts_off=k * B * 3,
                                              advance=(i == c.lv[-1]), **source)
            return masks[:5], lists, masks[5] if c.prev_upconv1 is not None else masks[0], None
        # a level whose heads run on the fused kernels needs no pixel lists: its three counts (upconv0, upconv1, wavelet:
        # specs 1, 3, 4) are accumulated by the mask launch itself
        counted = (c.all_nnz[len(c.counters)], [1, 3, 4]) if (sparse and i in c.lv and _fused_heads(c.sw, c1.weight.shape[0])) else None
        if i == 4 and not forced:
            masks = self._ones_masks(c.dev, B, h, w)
        elif forced:
            masks = S.dilate_multi(self._base_mask(c.force, i, B, h, w, c.dev).contiguous(), SPECS, counts=counted)
        elif state is None and c.sw.unfused_masks and B == 1:   # the three-launch form (parity tests)
            mask = S.mask_threshold(yh, S.minmax(yl), c.thresh)
            masks = [m.unsqueeze(0) for m in S.dilate_multi(mask, SPECS)]
            counted = None
        else:
            masks = [m.reshape(B, *m.shape[-2:]) for m in S.mask_level(yl, yh, c.thresh, SPECS, counts=counted)]
        return masks, None, masks[0], counted

    def _range_keys(self, c, want_keys, width):
        """state.keys when the next level's mask launch wants this level's LL range and the head kernels of this width fold it."""
        c.keys_armed = want_keys and ops.head_level_folds_range_keys(width)
        return c.state.keys if c.keys_armed else None

    def _record_ops(self, c, i, h, w, c0, c1, nnz=None, dense_cin=None):
        """Level i's part of the op model: its static operations and, for a sparse level (dense_cin None), the layer widths that
        resolve_total_ops multiplies with the pixel counts.  dense_cin: the in-channels of the two trunk layers as they ran."""
        c0, c1 = c0.weight, c1.weight
        if dense_cin is None:
            hp = self.convs[("waveconv", i, 1)]
            c.static_ops[i] = level_static_ops(i, h, w, True)
            c.counters.append((i, nnz, (c0.shape[1], c0.shape[0]), (c1.shape[1], c1.shape[0]),
                               (hp[0].conv.weight.shape[1], hp[0].conv.weight.shape[0]), (hp[2].conv.weight.shape[1], 3)))
        else:
            hds = [self.convs[("waveconv", i, j)] for j in ([0] if i == 4 else []) + [-1, 1]]
            c.static_ops[i] = level_static_ops(
                i, h, w, False, ((dense_cin[0], c0.shape[0]), (dense_cin[1], c1.shape[0])),
                [(hd[0].conv.weight.shape[1], hd[0].conv.weight.shape[0], hd[2].conv.weight.shape[1],
                  hd[2].conv.weight.shape[0]) for hd in hds])

    def _dense_level(self, c, i, c0, c1, src, yl, wavelet, fused, want_keys):
        """A dense level (the coarsest one, and any level outside sparse_scales) -> (activations, yl, yh, (next yl, disp) or
        None).  fused: the heads run on the fused head kernels, selecting on the wavelet mask and running the synthesis;
        else stacked 1x1 + 3x3 heads, yh multiplied by the mask, synthesis left to the caller."""
        h, w = src.shape[-2:]
        if i == 4 and self._edge is not None:     # level 4 on the encoder's pre-activation
            xd = ops.conv2d_pre_activated(src, self._edge.pre(), c0.weight, c0.bias, pad="reflect", act="elu")
        else:
            xd = ops.conv2d_fused(src, c0.weight, c0.bias, pad="reflect", act="elu")
        skip = c.feats[i - 1] if self.use_skips else None
        ux = ops.conv2d_fused(xd, c1.weight, c1.bias, x2=skip, up1=2, pad="reflect", act="elu")
        self._record_ops(c, i, h, w, c0, c1, dense_cin=(src.shape[1], xd.shape[1] + (0 if skip is None else skip.shape[1])))
        if fused:
            # the inference form of the heads (chained 1x1 -> tap-partial GEMMs, then one pass of 9-tap gather + sigmoid +
            # combine + Haar synthesis + clamp: 3 launches instead of 5; the all-ones wavelet mask of level 4 needs no multiply)
            keys = self._range_keys(c, want_keys, ux.shape[1])
            res = ops.head_fused_level_nograd(
                ux, _unpack(self.convs[("waveconv", i, 1)]), _unpack(self.convs[("waveconv", i, -1)]), scale=2.0 ** (i - 1),
                yl=None if i == 4 else yl, disp_scale=1.0 / 2 ** (i - 1), clamp01=True,
                head_ll=_unpack(self.convs[("waveconv", 4, 0)]) if i == 4 else None, scale_ll=2.0 ** 4,
                yh_mask=None if i == 4 else wavelet.contiguous(), range_keys=keys)
            if i == 4:
                yh, yl_next, disp, yl = res
            else:
                yh, yl_next, disp = res
            return ux, yl, yh, (yl_next, disp)
        ll_new, yh = self._dense_coefficients(ux, i, with_ll=(i == 4))
        if i == 4:
            yl = ll_new
        else:
            yh = yh * wavelet.reshape(c.B, 1, 1, 2 * h, 2 * w)   # reference :272 (all ones at i == 4)
        return ux, yl, yh, None

    def _sparse_level(self, c, i, c0, c1, src, yl, masks, lists, lowres_in, counted, want_keys):
        """A sparse level in the form the switches and the LevelState chose -> (activations, yh, (next yl, disp) or None)."""
        assert self.use_skips and i > 0 and yl is not None
        lowres, upconv0, upsample_m, upconv1, wavelet = masks
        B, state = c.B, c.state
        h, w = src.shape[-2:]
        H2, W2 = 2 * h, 2 * w
        C0, C1_ = c0.weight.shape[0], c1.weight.shape[0]
        nnz = None
        if state is None:
            nnz = c.all_nnz[len(c.counters)]
            if counted is None:     # pixel lists (gather-GEMM form) and / or counts by stream compaction
                (co0, co1, cow), nnz = S.compact_multi([upconv0, upconv1, wavelet], nnz_out=nnz)   # coords [B,npix], counts [B,3]
        x0 = c.planes.take(B, C0, h, w)
        skip = c.feats[i - 1].contiguous()
        x1 = c.planes.take(B, C1_, H2, W2)
        if c.sw.tiles:
            # several frames: the trunk convolutions run on the dense Winograd / MFMA kernels over the pixel TILES
            # that contain active pixels (tile list built on the device), input support and output mask folded
            # into the patch gather / the epilogue -- same values as the gather-GEMM, dense-kernel throughput
            tiles0, tiles1 = (lists[1], lists[3]) if lists is not None else (None, None)
            ops._conv_fwd_raw(src, None, ops.pack_weights(c0.weight), c0.bias, C0, 3, "reflect", "elu", 0.0, 1,
                              ops.pack_weights_wino(c0.weight), in_mask=lowres_in, out_mask=upconv0, out=x0, out_tiles=tiles0)
            ops._conv_fwd_raw(x0, skip, ops.pack_weights(c1.weight), c1.bias, C1_, 3, "reflect", "elu", 0.0, 2,
                              ops.pack_weights_wino(c1.weight), in_mask=upsample_m, out_mask=upconv1, out=x1,
                              in_mask_2x2=True,   # MaxPool5(upsample(m)) = upsample(MaxPool3(m)): constant on 2x2 blocks
                              out_tiles=tiles1)
        else:
            S.sparse_conv(x0, src, ops.pack_weights(c0.weight), c0.bias, C0, 3, co0, nnz.data_ptr(), h * w,
                          in_mask=lowres, pad="reflect", act="elu", nnz_stride=3)
            S.sparse_conv(x1, x0, ops.pack_weights(c1.weight), c1.bias, C1_, 3, co1, nnz.data_ptr() + 4, H2 * W2,
                          x2=skip, up1=2, in_mask=upsample_m, pad="reflect", act="elu", nnz_stride=3)
        hp, hn = self.convs[("waveconv", i, 1)], self.convs[("waveconv", i, -1)]
        synthesis = None
        if _fused_heads(c.sw, C1_):
            # heads of the tile mode: the dense fused head kernels (chained 1x1 -> tap-partial 3x3 -> sigmoid -> Haar
            # synthesis) with the wavelet mask applied to yh in their epilogue.  Same values as the gather form: every
            # 3x3 neighbour of a wavelet-mask pixel (reflection included) lies inside upconv1 = its radius-1 dilation,
            # where x1 holds the sparse activations, so the mid channels those taps read are the ones layers.py:405
            # computes; mid values outside the support are never read by a surviving output.
            keys = self._range_keys(c, want_keys, C1_)
            yh, yl_next, disp = ops.head_fused_level_nograd(x1, _unpack(hp), _unpack(hn), scale=2.0 ** (i - 1), yl=yl,
                                                            disp_scale=1.0 / 2 ** (i - 1), clamp01=True,
                                                            yh_mask=wavelet.contiguous(),
                                                            run_mask=upconv1 if state is not None else None, range_keys=keys)
            synthesis = (yl_next, disp)
        else:
            # heads: stacked 1x1 + LeakyReLU on the upconv1 support, dual 3x3 + sigmoid on the wavelet mask
            Cm = hp[0].conv.weight.shape[0]
            wstack, bstack = ops.stacked_pack([hp[0].conv.weight, hn[0].conv.weight], [hp[0].conv.bias, hn[0].conv.bias])
            mid = c.planes.take(B, 2 * Cm, H2, W2)
            S.sparse_conv(mid, x1, wstack, bstack, 2 * Cm, 1, co1, nnz.data_ptr() + 4, H2 * W2, act="leaky", slope=0.1,
                          nnz_stride=3)
            yh_d = c.planes.take(B, 3, H2, W2)
            S.sparse_conv(yh_d, mid, ops.pack_weights(hp[2].conv.weight), hp[2].conv.bias, 3, 3, cow,
                          nnz.data_ptr() + 8, H2 * W2, in_mask=upconv1, pad="reflect", act="sigmoid",
                          out_scale=2.0 ** (i - 1), c1=Cm, c1_off=0, wp2=ops.pack_weights(hn[2].conv.weight),
                          bias2=hn[2].conv.bias, c1_off2=Cm, nnz_stride=3)
            yh = yh_d.unsqueeze(1)
        self._record_ops(c, i, h, w, c0, c1, nnz=nnz)
        return x1, yh, synthesis

    @staticmethod
    def _host_op_model(out, counters, static_ops, state=None):
        # ---- the reference's op model needs the pixel counts as python ints.  They are copied to pinned host memory
        # asynchronously and turned into the `total_ops` entries on first access: the forward itself never waits for the GPU
        out = S.LazyOpsDict(out)
        if state is not None:      # work-list form: the counts wait in the ring slot of this forward (number state.seq - 1)
            fetch = state.counts_fetcher(state.seq - 1)
        else:
            fetch = S.counts_to_host([nnz for (_lvl, nnz, *_rest) in counters])
        levels = [lvl for (lvl, *_rest) in counters]

        def resolver():
            flat = fetch()                                      # per level: B * 3 counts, frame-major
            B = len(flat[0]) // 3 if flat else 1
            frames = []
            for f in range(B):
                resolved = {lvl: cnt[3 * f:3 * f + 3] for lvl, cnt in zip(levels, flat)}
                frames.append(resolve_total_ops(static_ops, counters, resolved))
            if len(frames) == 1:
                per_scale, total = frames[0]
                res = {("total_ops", sc): n for sc, n in per_scale.items()}
                res["total_ops"] = total
            else:                                               # batched decode: one integer per frame
                res = {("total_ops", sc): [fr[0][sc] for fr in frames] for sc in frames[0][0]}
                res["total_ops"] = [fr[1] for fr in frames]
            return res

        out.set_lazy([("total_ops", i - 1) for i in static_ops] + ["total_ops"], resolver)
        return out
