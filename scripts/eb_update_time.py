"""wall time of EntropyBottleneck.update() at C = 192 beside a torch-eager restatement of the same steps on the same GPU"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flashgmm_amd import EntropyBottleneck, ops  # noqa: E402

DEV = "cuda:0"


@torch.no_grad()
def eager_update(eb, update_quantiles):
    f = lambda y: eb._logits_cumulative(y, stop_gradient=True)  # noqa: E731
    q = eb.quantiles.detach().clone()
    steps = 0
    if update_quantiles:
        Cn = eb.channels
        t = eb.target.reshape(1, 1, 3).expand(Cn, 1, 3)
        lo, hi = torch.full((Cn, 1, 3), -1e5, device=DEV), torch.full((Cn, 1, 3), 1e5, device=DEV)
        lo = torch.where(t <= f(hi), lo, hi)
        hi = torch.where(f(lo) <= t, hi, lo)
        for _ in range(256):
            mid = (lo + hi) / 2
            done = (mid == lo) | (mid == hi)
            if bool(done.all()):
                break
            steps += 1
            fv = f(mid)
            lo, hi = torch.where(~done & (fv <= t), mid, lo), torch.where(~done & (fv >= t), mid, hi)
        q = (lo + hi) / 2
    med = q[:, 0, 1]
    minima = torch.clamp(torch.ceil(med - q[:, 0, 0]).int(), min=0)
    maxima = torch.clamp(torch.ceil(q[:, 0, 2] - med).int(), min=0)
    start, length = med - minima, maxima + minima + 1
    n = int(length.max().item())
    s = (torch.arange(n, device=DEV)[None, :] + start[:, None])[:, None, :]
    lo_, up_ = f(s - 0.5), f(s + 0.5)
    flip = (lo_ + up_) > 0
    L = torch.where(flip, torch.sigmoid(-lo_) - torch.sigmoid(-up_), torch.sigmoid(up_) - torch.sigmoid(lo_))[:, 0]
    tail = torch.sigmoid(lo_[:, 0, 0]) + torch.sigmoid(-up_[:, 0].gather(1, (length - 1).long()[:, None])[:, 0])
    L, tail, length = L.cpu().numpy(), tail.cpu().numpy(), length.cpu().numpy()
    cdf = np.zeros((eb.channels, n + 2), np.int32)
    for c in range(eb.channels):
        cdf[c, :length[c] + 2] = ops.pmf_to_quantized_cdf(np.concatenate([L[c, :length[c]], tail[c:c + 1]]), 16)
    return torch.from_numpy(cdf).to(DEV), steps


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return sorted(out)


def main():
    torch.manual_seed(0)
    eb = EntropyBottleneck(192).to(DEV)
    with torch.no_grad():
        for n, p in eb.named_parameters():
            if "matrix" in n:
                p.add_(0.3 * torch.randn_like(p))
            elif "factor" in n:
                p.copy_(0.5 * torch.randn_like(p))
    eb.update(force=True, update_quantiles=True)
    print("C = 192, pmf_length min / median / max:", min(eb.update_report["pmf_length"]), int(np.median(eb.update_report["pmf_length"])), max(eb.update_report["pmf_length"]))
    for uq in (True, False):
        mine = timed(lambda: eb.update(force=True, update_quantiles=uq))
        cdf, steps = eager_update(eb, uq)
        same = int((cdf == eb._quantized_cdf).all(1).sum())
        eager = timed(lambda: eager_update(eb, uq))
        print(f"update_quantiles={uq}: update() {mine[0]:.2f} / {mine[len(mine) // 2]:.2f} ms (min / median of {len(mine)}); torch eager {eager[0]:.2f} / {eager[len(eager) // 2]:.2f} ms"
              f" ({steps} bisection steps); tables equal in {same} of 192 channels")


if __name__ == "__main__":
    main()
