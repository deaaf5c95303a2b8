"""CPU emulation of the vocoder's fp16 mode (include/ctts.h, "HiFi-GAN vocoder, fp16 mode") on the folded weights of
tests/hifigan_restate.py - a helper of the half-precision tests, not a test.  It rounds exactly where the contract rounds:

  weights      folded (in the dtype fold_state_dict was asked for: float32 is the contract's), rounded once to fp16; biases untouched
  mel          rounded to fp16 when conv_pre reads it
  operand      fp16(leaky_relu(float32(x))) of every convolution but conv_post
  stored       every layer's result, fp16(beta * out + alpha * (acc + bias + R)), saturated to +-65504 - `xs` included
  conv_post    reads the fp16 activations, everything else (leaky_relu, unrounded weights, tanh) in the accumulation dtype

and takes the accumulation dtype as a parameter: float64 (the rounding alone) or float32 (what the kernels accumulate in; the CPU's
summation order is not the MFMA's, which is why the tests compare both with float64 and never with each other).  `reverse_channels`
flips the input-channel order of every convolution: the same arithmetic in another summation order.  `rounding=False` switches every
rounding off: the emulation then is hifigan_restate.generator_forward in its own launch structure (xs accumulated by alpha / beta)."""
import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.1
FP16_MAX = 65504.0


def round_half(x, on=True):
    """x rounded to fp16 (round to nearest even, saturated to +-65504), returned in x's dtype"""
    if not on:
        return x
    return x.clamp(-FP16_MAX, FP16_MAX).to(torch.float16).to(x.dtype)


def _operand(x, slope, on):
    """fp16(leaky_relu(float32(x), slope)) in x's dtype: x holds fp16 values, the product with the fp32 slope is rounded to fp32, then to fp16"""
    if not on:
        return x if slope is None else F.leaky_relu(x, slope)
    if slope is None:
        return round_half(x)
    x32 = x.float()
    return round_half(torch.where(x32 > 0, x32, x32 * slope)).to(x.dtype)


def _conv(x, w, k, d, rev, transposed_u=0):
    if rev:
        x = x.flip(1)
        w = w.flip(0) if transposed_u else w.flip(1)
    if transposed_u:
        return F.conv_transpose1d(x, w, None, transposed_u, (k - transposed_u) // 2)
    return F.conv1d(x, w, None, 1, d * (k - 1) // 2, d)


def generator_forward_half(W, h, mel, acc_dtype=torch.float64, rounding=True, reverse_channels=False):
    """W: hifigan_restate.fold_state_dict(sd, dtype=torch.float32) (or float64 with rounding=False); mel [B, 80, T] -> wav [B, 1, 256 T]
    in acc_dtype.  Channel-first tensors, as the restatement."""
    on, rev = rounding, reverse_channels

    def wq(name):
        w, b = W[name]
        return round_half(w, on).to(acc_dtype), b.to(acc_dtype)[None, :, None]

    def layer(x, name, k, d=1, slope=LRELU_SLOPE, u=0, R=None, old=None, alpha=1.0, beta=0.0):
        w, b = wq(name)
        v = _conv(_operand(x, slope, on), w, k, d, rev, u) + b
        if R is not None:
            v = v + R
        v = alpha * v
        if beta != 0.0:
            v = beta * old + v
        return round_half(v, on)

    nk = len(h["resblock_kernel_sizes"])
    x = layer(mel.to(acc_dtype), "conv_pre", 7, slope=None)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = layer(x, f"ups.{i}", k, u=u)
        xs = None
        for j, (kr, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            cur, p = x, f"resblocks.{i * nk + j}"
            for l, d in enumerate(dil[:3]):
                t = layer(cur, f"{p}.convs1.{l}", kr, d)
                if l < 2:
                    cur = layer(t, f"{p}.convs2.{l}", kr, 1, R=cur)
                else:
                    last = j == nk - 1
                    xs = layer(t, f"{p}.convs2.{l}", kr, 1, R=cur, old=xs, alpha=1.0 / nk if last else 1.0,
                               beta=0.0 if j == 0 else (1.0 / nk if last else 1.0))
        x = xs
    w, b = W["conv_post"]
    x = F.leaky_relu(x)
    if rev:
        x, w = x.flip(1), w.flip(1)
    return torch.tanh(F.conv1d(x, w.to(acc_dtype), b.to(acc_dtype), 1, 3))
