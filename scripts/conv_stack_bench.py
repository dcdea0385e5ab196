"""The dense convolution layers of header section 5d and the transposed ones of 5e, measured (profiles/conv_stack.md,
profiles/conv_transposed.md): ConvStack (fgmm_conv.hip: one launch per layer,
activation and PixelShuffle(2) folded into the store) against the torch modules it replaces (MIOpen, warmed) on
  - the checkerboard GMM model's h_s (N = 192, M = 320: five 3x3 layers, two with PixelShuffle(2)) on z_hat [24, 192, 8, 12] and [1, 192, 8, 12];
  - ELIC's last channel-context module (three 5x5 layers, 128 -> 224 -> 128 -> 384, ReLU) on [1, 128, 135, 240];
  - ELIC's h_s (N = 192: ConvTranspose2d 5x5 stride 2, 192 -> 192 -> 288, ReLU, then 3x3 stride 1 to 384; ConvStack(transposed=True),
    fgmm_deconv.hip) on z_hat [1, 192, 34, 60] (ELIC-4K) and [16, 192, 34, 60] - and, for its two stride-2 layers alone, the third path
    "emulation": the same layers as a dense 3x3 to 4 c_out channels with zero-padded sub-kernels and the PixelShuffle(2) store on
    section 5d's kernel, the 36 products per channel the phase split's 25 have to beat.

GPU time by device events on the current stream: a sample is `inner` back-to-back calls between two events, divided by `inner`; the two
paths alternate sample by sample in one process; the median and the minimum of `samples` samples after `warm` warm-up samples of each.
The share of the f32 MFMA roof (157.3 TF, as profiles/r06_head_kernel.md) counts the multiply-adds the definition needs,
2 * c_out * c_in * k^2 per position and layer.  Needs a GPU: fails without one.
With `--arithmetic bf16x6` the bf16x6 form (fgmm_conv16.hip; profiles/conv_bf16x6.md) joins the alternation on the workloads of Conv2d
layers: the whole call - per layer the split, conv16_kernel and the flagged-items launch - against the exact handle and torch in the same
process, and conv16_kernel alone (the device durations torch's profiler records for it over `samples` calls, summed per call) as a share
of the BF16 roof (419.5 TF of six part products per product, as profiles/ckbd_context_bf16x6.md).
With `--grad` (profiles/conv_grad.md) the script measures ONLY forward + backward under autograd - ConvStack on an input that requires
grad (header section 5f: ops.conv_layer per layer, the weights packed at every call, fgmm_conv.hip's gradient staging and fgmm_conv_grad.hip)
against the torch modules' forward + backward (MIOpen), gradients of the input and of every parameter - on the two h_s shapes and the
channel context, alternating sample by sample as above; and the largest difference of a gradient of either path from float64 autograd of
the same modules (and of the two paths from each other), relative to that gradient's largest element.
With `--trace` (profiles/conv_grad.md, the last section) nothing is timed: on the same three workloads the script names where the library's
binary32 forward and float64 autograd take DIFFERENT activation branches - per layer the number of such elements, and the first one's
index, its float64 pre-activation and the library's output - and gives the gradients' largest difference from float64 twice: against
float64 with its own branches, and against float64 made to take the library's branch at every element.
usage: python scripts/conv_stack_bench.py [samples=20] [inner=5] [warm=3] [--arithmetic bf16x6 | --grad | --trace]"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flashgmm_amd import ConvStack  # noqa: E402

ARITH = "f32"
if "--arithmetic" in sys.argv:
    at = sys.argv.index("--arithmetic")
    ARITH = sys.argv[at + 1]
    del sys.argv[at:at + 2]
assert ARITH in ("f32", "bf16x6"), ARITH
GRAD, TRACE = "--grad" in sys.argv, "--trace" in sys.argv
for flag in ("--grad", "--trace"):
    if flag in sys.argv:
        sys.argv.remove(flag)
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 20
inner = int(sys.argv[2]) if len(sys.argv) > 2 else 5
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 3
ROOF_TF, ROOF16_TF = 157.3, 419.5
assert torch.cuda.is_available(), "scripts/conv_stack_bench.py needs a GPU"
dev = "cuda:0"
torch.manual_seed(1)
conv3, conv5 = lambda i, o: nn.Conv2d(i, o, 3, padding=1), lambda i, o: nn.Conv2d(i, o, 5, padding=2)
subpel = lambda i, o: nn.Sequential(nn.Conv2d(i, o * 4, 3, padding=1), nn.PixelShuffle(2))
N_, M_ = 192, 320
h_s = nn.Sequential(conv3(N_, M_), nn.LeakyReLU(), subpel(M_, M_), nn.LeakyReLU(), conv3(M_, M_ * 3 // 2), nn.LeakyReLU(), subpel(M_ * 3 // 2, M_ * 3 // 2),
                    nn.LeakyReLU(), conv3(M_ * 3 // 2, M_ * 2)).to(dev)
cc = nn.Sequential(conv5(128, 224), nn.ReLU(), conv5(224, 128), nn.ReLU(), conv5(128, 384)).to(dev)
deconv = lambda i, o, k, s: nn.ConvTranspose2d(i, o, k, stride=s, padding=k // 2, output_padding=s - 1)
elic_h_s = nn.Sequential(deconv(N_, N_, 5, 2), nn.ReLU(), deconv(N_, N_ * 3 // 2, 5, 2), nn.ReLU(), deconv(N_ * 3 // 2, N_ * 2, 3, 1)).to(dev)


def emulation(net):
    """the stride-2 5x5 transposed layers of net as Conv2d(c_in, 4 c_out, 3, padding=1) + PixelShuffle(2): output channel 4 o + 2 pr + pc
    holds phase (pr, pc)'s taps at their input offsets, zeros elsewhere"""
    taps = lambda par: [(a, (par + a - 2) // 2) for a in range(5) if (par + a) % 2 == 0]
    mods = []
    for m in net:
        if not isinstance(m, nn.ConvTranspose2d):
            mods.append(m)
            continue
        conv = nn.Conv2d(m.in_channels, 4 * m.out_channels, 3, padding=1).to(dev)
        with torch.no_grad():
            conv.weight.zero_()
            conv.bias.copy_(m.bias.repeat_interleave(4))
            for pr in (0, 1):
                for pc in (0, 1):
                    for a, dr in taps(pr):
                        for b, dc in taps(pc):
                            conv.weight[2 * pr + pc::4, :, dr + 1, dc + 1] = m.weight[:, :, 4 - a, 4 - b].t()
        mods.append(nn.Sequential(conv, nn.PixelShuffle(2)))
    return nn.Sequential(*mods)


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, r


def kernel_alone_ms(fn, name, calls):
    """the device time of the kernels whose name holds `name`, per call of fn, from torch's profiler (None: it recorded none)"""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    us = [float(getattr(e, "device_time_total", 0) or getattr(e, "cuda_time_total", 0)) for e in prof.key_averages() if name in e.key]
    return round(sum(us) / calls / 1e3, 5) if us and sum(us) > 0 else None


def flops(net, x):
    """multiply-adds x 2 of every convolution of net on x, by the shapes"""
    total, hooks = [0.0], []
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            hooks.append(m.register_forward_hook(lambda m, i, o: total.__setitem__(0, total[0] + 2.0 * o.numel() * m.in_channels * m.kernel_size[0] ** 2)))
        if isinstance(m, nn.ConvTranspose2d):  # k^2 products per input position and channel pair
            hooks.append(m.register_forward_hook(lambda m, i, o: total.__setitem__(0, total[0] + 2.0 * i[0].numel() * m.out_channels * m.kernel_size[0] ** 2)))
    with torch.no_grad():
        net(x)
    for hk in hooks:
        hk.remove()
    return total[0]


out = {"compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "samples": samples, "calls_per_sample": inner, "warmup_samples": warm,
       "roof_tf": ROOF_TF}
def grad_leg(name, net, shape):
    """forward + backward of ConvStack(net) against the torch modules'; and both paths' gradients against float64 autograd of the same modules"""
    import copy

    x, op, params = torch.randn(shape, device=dev, requires_grad=True), ConvStack(net), list(net.parameters())
    g = torch.randn_like(net(x))
    paths = {"kernel": lambda: torch.autograd.grad(op(x), [x] + params, g), "torch": lambda: torch.autograd.grad(net(x), [x] + params, g)}
    for _ in range(warm):
        for fn in paths.values():
            sample(fn)
    t = {k: [] for k in paths}
    for _ in range(samples):
        for k, fn in paths.items():
            t[k].append(sample(fn)[0])
    res = {k: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(np.min(v)), 5)} for k, v in t.items()}
    res["kernel_over_torch"] = round(res["kernel"]["median_ms"] / res["torch"]["median_ms"], 4)
    net64, x64 = copy.deepcopy(net).double(), x.detach().double().requires_grad_(True)
    exact = torch.autograd.grad(net64(x64), [x64] + list(net64.parameters()), g.double())
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.abs().max())  # of a gradient's largest element
    names = ["input"] + [n for n, _ in net.named_parameters()]
    got = {k: fn() for k, fn in paths.items()}
    for k in paths:  # every gradient of the path against float64: the largest, and whose it is
        worst = max(range(len(names)), key=lambda i: rel(got[k][i], exact[i]))
        res[k]["max_rel_grad_diff_to_float64"] = {"gradient": names[worst], "value": rel(got[k][worst], exact[worst])}
    res["max_rel_grad_diff_to_torch"] = max(rel(a, b) for a, b in zip(got["kernel"], got["torch"]))
    return res


def trace_leg(net, shape):
    """the activation branches in which the library's forward and float64 autograd differ, and the gradients with and without them"""
    import copy

    from flashgmm_amd.ops import conv_layer

    layers, x = ConvStack.check(list(net)), torch.randn(shape, device=dev, requires_grad=True)
    outs, v = [], x
    for conv, act, slope, shuffle in layers:  # the library's layers one by one: an output's sign is its pre-activation's (slope >= 0)
        v = conv_layer(v, conv.weight, conv.bias, ("none", "leaky_relu", "relu")[act], slope, shuffle)
        outs.append(v.detach())
    g = torch.randn_like(v)
    got = torch.autograd.grad(v, [x] + list(net.parameters()), g)
    net64 = copy.deepcopy(net).double()

    def float64(branches):
        """-> the pre-activations and the gradients of the float64 stack; branches: None = its own, else per layer the mask of the positive branch"""
        x64, pre = x.detach().double().requires_grad_(True), []
        v = x64
        for j, (conv, act, slope, shuffle) in enumerate(ConvStack.check(list(net64))):
            z = nn.functional.pixel_shuffle(nn.functional.conv2d(v, conv.weight, conv.bias, padding=conv.kernel_size[0] // 2), shuffle)
            pre.append(z.detach())
            v = z if act == 0 else torch.where(z > 0 if branches is None else branches[j], z, z * slope)
        return pre, torch.autograd.grad(v, [x64] + list(net64.parameters()), g.double())

    (pre, own), (_, forced) = float64(None), float64([o > 0 for o in outs])
    rel = lambda a, b: max(float((u.double() - w).abs().max() / w.abs().max()) for u, w in zip(a, b))  # of a gradient's largest element
    res = {"differing_branches_per_layer": [], "max_rel_grad_diff_to_float64": rel(got, own), "max_rel_grad_diff_to_float64_on_the_library_s_branches": rel(got, forced)}
    for j, (z, o, (_, act, *_)) in enumerate(zip(pre, outs, layers)):
        at = torch.nonzero(((z > 0) != (o > 0)).flatten() & bool(act))[:, 0]
        res["differing_branches_per_layer"].append(int(at.numel()))
        if at.numel() and "first" not in res:
            res["first"] = {"layer": j, "flat_index": int(at[0]), "float64_pre_activation": float(z.flatten()[at[0]]), "library_output": float(o.flatten()[at[0]])}
    return res


if GRAD or TRACE:
    for name, net, shape in (("h_s N=24", h_s, (24, N_, 8, 12)), ("h_s N=1", h_s, (1, N_, 8, 12)), ("channel_context", cc, (1, 128, 135, 240))):
        out[name + (" forward+backward" if GRAD else " branches")] = grad_leg(name, net, shape) if GRAD else trace_leg(net, shape)
    print(json.dumps(out))
    sys.exit(0)
for name, net, shape in (("h_s N=24", h_s, (24, N_, 8, 12)), ("h_s N=1", h_s, (1, N_, 8, 12)), ("channel_context", cc, (1, 128, 135, 240)),
                         ("elic_h_s N=1", elic_h_s, (1, N_, 34, 60)), ("elic_h_s N=16", elic_h_s, (16, N_, 34, 60)),
                         ("elic_h_s stride-2 layers N=1", elic_h_s[:4], (1, N_, 34, 60)), ("elic_h_s stride-2 layers N=16", elic_h_s[:4], (16, N_, 34, 60))):
    x, op = torch.randn(shape, device=dev), ConvStack(net, transposed=True)

    def torch_path():
        with torch.no_grad():
            return net(x)

    paths = {"kernel": lambda: op(x), "torch": torch_path}
    if "stride-2" in name:
        emu = ConvStack(emulation(net))
        paths["emulation"] = lambda: emu(x)
    b16 = ARITH == "bf16x6" and not any(isinstance(m, nn.ConvTranspose2d) for m in net)
    if b16:
        op16 = ConvStack(net, arithmetic="bf16x6")
        paths["bf16x6"] = lambda: op16(x)
    for _ in range(warm):
        for fn in paths.values():
            sample(fn)
    t = {k: [] for k in paths}
    for _ in range(samples):
        for k, fn in paths.items():
            t[k].append(sample(fn)[0])
    res = {k: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(np.min(v)), 5)} for k, v in t.items()}
    res["gflop"] = round(flops(net, x) / 1e9, 3)
    res["kernel"]["frac_of_roof"] = round(res["gflop"] / res["kernel"]["median_ms"] / ROOF_TF, 4)
    res["kernel_over_torch"] = round(res["kernel"]["median_ms"] / res["torch"]["median_ms"], 4)
    res["max_abs_diff_to_torch"] = float((torch_path() - op(x)).abs().max())
    if b16:
        res["bf16x6"]["tflops"] = round(res["gflop"] / res["bf16x6"]["median_ms"], 2)
        res["bf16x6"]["frac_of_bf16_roof"] = round(res["gflop"] / res["bf16x6"]["median_ms"] / ROOF16_TF, 4)
        res["kernel_over_bf16x6"] = round(res["kernel"]["median_ms"] / res["bf16x6"]["median_ms"], 4)
        res["bf16x6_over_torch"] = round(res["bf16x6"]["median_ms"] / res["torch"]["median_ms"], 4)
        res["max_abs_diff_bf16x6_to_kernel"] = float((op16(x) - op(x)).abs().max())
        alone = kernel_alone_ms(lambda: op16(x), "conv16_kernel", samples)
        res["conv16_kernel_alone"] = {"ms": alone, "frac_of_bf16_roof": alone and round(res["gflop"] / alone / ROOF16_TF, 4)}
    if "emulation" in paths:
        res["kernel_over_emulation"] = round(res["kernel"]["median_ms"] / res["emulation"]["median_ms"], 4)
        res["emulation_max_abs_diff_to_torch"] = float((torch_path() - emu(x)).abs().max())
    out[name] = res
print(json.dumps(out))
