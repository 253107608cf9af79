"""Where does the swin benchmark's task token move when the LayerNorm changes
in the last fp32 bits?  swin-tiny, eval, bf16 autocast, tap = input of the
last stage ([B, 49, 768] bf16), token = mean over the batch.  Three routes:
fused (add_ln.hip), eager (torch LN), exact (eager with the block norms
evaluated in float64 and rounded once to fp32)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

from flreid_amd.models.swin import SwinBlock, swin_reid

torch.manual_seed(0)
model = swin_reid("tiny", num_classes=1000, neck="bnneck").cuda().eval()
x = torch.randn(128, 3, 224, 224, device="cuda")


class ExactLN(nn.LayerNorm):
    def forward(self, t):
        d = t.double()
        mean = d.mean(-1, keepdim=True)
        var = ((d - mean) ** 2).mean(-1, keepdim=True)
        y = (d - mean) * (var + self.eps).rsqrt() * self.weight.double() \
            + self.bias.double()
        return y.float()


def tap(route):
    os.environ["FLREID_SWIN_ADD_LN"] = "1" if route == "fused" else "0"
    cls = ExactLN if route == "exact" else nn.LayerNorm
    for m in model.modules():
        if isinstance(m, SwinBlock):
            m.norm1.__class__ = cls
            m.norm2.__class__ = cls
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        _, t = model.run_stages(x, 0, tap=4)
    return t.float()


taps = {r: tap(r) for r in ("fused", "eager", "exact")}
assert torch.equal(taps["fused"], tap("fused"))
for a, b in (("fused", "eager"), ("eager", "exact"), ("fused", "exact")):
    ta, tb = taps[a], taps[b]
    d = (ta - tb).abs()
    tok = (ta.mean(0) - tb.mean(0)).abs()
    ref = tb.mean(0)
    print("%s vs %s: taps differ in %.1f%% of elements, rms|d|/rms = %.3e; "
          "token max|d| = %.3e, max|d|/max|token| = %.3e, rms ratio = %.3e"
          % (a, b, 100 * float((d > 0).float().mean()),
             float(d.pow(2).mean().sqrt() / tb.pow(2).mean().sqrt()),
             float(tok.max()), float(tok.max() / ref.abs().max()),
             float(tok.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())))
