"""CPU reference of the opt-in bf16 trunk precision (include/wmd.h, wmd_conv_bf16_fwd), composed from the oracle's public
blocks exactly as oracle.decoder_ref.kitti_wave_decoder composes them: only the eight trunk ConvBlocks differ.

  q(v)       fp32 -> bf16 round-to-nearest-even (torch.Tensor.bfloat16), returned as fp32
  terms = 1  y = act( sum_k q(x_k) q(w_k) + bias )
  terms = 3  y = act( sum_k [ q(x_k) q(w_k) + q(x_k) q(w_k - q(w_k)) + q(x_k - q(x_k)) q(w_k) ] + bias )
Products of two bf16 values are exact in fp32; the sums run in fp32 (acc64: in fp64, for the spread between two correct
summation orders); bias and activation in fp32."""
import torch
import torch.nn.functional as F

from oracle import decoder_ref as R


def q(v):
    return v.bfloat16().float()


def _act(z, act, slope):
    if act == "elu":
        return F.elu(z)
    if act == "leaky":
        return F.leaky_relu(z, slope)
    assert act in ("none", None)
    return z


def conv_block_bf16(x, w, b, terms, acc64=False, pad="reflect", act="elu", slope=0.0):
    """x: the (already upsampled / concatenated) fp32 input of the block, w [Cout,Cin,3,3], b [Cout] or None."""
    assert terms in (1, 3)
    xp = R.pad1(x, pad)
    xh, wh = q(xp), q(w)
    dt = torch.float64 if acc64 else torch.float32
    z = F.conv2d(xh.to(dt), wh.to(dt))
    if terms == 3:
        xl, wl = q(xp - xh), q(w - wh)
        z = z + F.conv2d(xh.to(dt), wl.to(dt)) + F.conv2d(xl.to(dt), wh.to(dt))
    z = z.float()
    if b is not None:
        z = z + b.view(1, -1, 1, 1)
    return _act(z, act, slope)


def kitti_wave_decoder_bf16(feats, sd, terms, acc64=False):
    keys = R.kitti_wave_keys()
    out = {}
    x = feats[-1]
    yl = None

    def block(x, i, j):
        p = "decoder.%d" % keys[("upconv", i, j)]
        return conv_block_bf16(x, sd[p + ".conv.conv.weight"], sd[p + ".conv.conv.bias"], terms, acc64)

    for i in range(4, 0, -1):
        x = block(x, i, 0)
        x = torch.cat([R.up2(x), feats[i - 1]], 1)
        x = block(x, i, 1)
        ll_new, yh = R.kitti_wave_coefficients(x, sd, keys, i, with_ll=(i == 4))
        if i == 4:
            yl = ll_new
        out[("wavelets", i - 1, "LL")] = yl
        out[("wavelets", i - 1, "LH")] = yh[:, :, 0]
        out[("wavelets", i - 1, "HL")] = yh[:, :, 1]
        out[("wavelets", i - 1, "HH")] = yh[:, :, 2]
        yl = R.haar_idwt(yl, yh)
        out[("disp", i - 1)] = torch.clamp(yl / 2 ** (i - 1), 0, 1)
    return out
