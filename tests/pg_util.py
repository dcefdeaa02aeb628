"""The float64 yardstick of the policy-gradient heads and the PPO loss (csrc/wsmg_pg_heads.hip), written with torch autograd on
the CPU, and the rule that turns it into a bar.

`eval_heads_ref` is habitat's CriticHead + the reference's DiagGaussian / patched Normal (common/distributions.py:21-29,42-57):
torch.distributions.Normal gives the log-probability and the entropy.  `ppo_loss_ref` is the clipped-surrogate loss of
habitat-baselines' PPO.update, restated (habitat is not a dependency).  Both take `dtype`: float64 is the oracle, float32 is the
"stock float32 torch composition" whose own distance from the oracle sets the bar of every compared quantity:

    bar = max(4 x |stock float32 - oracle|_max, 1e-6 x |oracle|_max)

4 x because the kernels add in another order; the second term is the floor for a quantity on which the float32 composition
happens to be exact (or nearly: a correctly rounded float32 number sits anywhere between 0 and half an ulp, 6e-8 relative, from the
float64 value, so 4 x a lucky 0.01 ulp is no bar a correct kernel could be held to).  Where the oracle is exactly zero the bar is
zero: the kernels must give exactly zero there too.  (Worded for the feature as a floor "where that error is zero"; it is
applied whenever 4 x the error falls below it, for the reason just given — profiles/pg_heads.txt counts the comparisons it decided.)

The masked means are written (x * w).sum() / w.sum() with w the 0 / 1 mask: on finite rows that is the mean over the selected
rows, a row left out gets the gradient 0 * (d loss / n) = 0, and with NO row selected the loss is 0 / 0 and every row's
gradient 0 * inf: NaN, which is what the kernels are held to.  (The kernels drop the rows a mask leaves out instead of
multiplying them, as aux_reduce does; on finite inputs the two agree.)"""
import math

import torch
import torch.nn.functional as F
from torch.distributions import Normal


def f32_scalar(v):
    """The float32 value a Python float becomes on its way through the C ABI (the oracle must see the same number)."""
    return float(torch.tensor(v, dtype=torch.float32))


def eval_heads_ref(x, wm, bm, logstd, wc, bc, action, dtype=torch.float64):
    """-> (value [B,1], logp [B], entropy 0-dim, mean [B,A]).  The arguments must already be leaves of `dtype` where a gradient
    is wanted; others are converted.  logstd is the [A, 1] parameter of DiagGaussian.logstd."""
    c = lambda t: t.to(dtype)      # noqa: E731
    mean = F.linear(c(x), c(wm), c(bm))
    scale = (torch.zeros_like(mean) + c(logstd).t().view(1, -1)).exp()
    dist = Normal(mean, scale, validate_args=False)
    logp = dist.log_prob(c(action)).sum(-1)
    entropy = dist.entropy().sum(-1).mean()
    value = F.linear(c(x), c(wc).view(1, -1), c(bc).view(1))
    return value, logp, entropy, mean


def eval_heads_run(inp, grads, dtype):
    """Forward + backward of eval_heads_ref in `dtype` from the float32 inputs `inp` = (x, wm, bm, logstd, wc, bc, action) with the
    upstream gradients `grads` = (g value [B,1] | None, g logp [B] | None, g entropy 0-dim | None).
    -> dict of value, logp, entropy, dx, dwm, dbm, dlogstd, dwc, dbc (a gradient nothing reaches is zeros)."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in inp[:6]]
    value, logp, entropy, _ = eval_heads_ref(*leaves, inp[6], dtype=dtype)
    total = sum((o * g.to(dtype)).sum() for o, g in zip((value, logp, entropy), grads) if g is not None)
    total.backward()
    out = dict(value=value.detach(), logp=logp.detach(), entropy=entropy.detach())
    for name, leaf in zip(("dx", "dwm", "dbm", "dlogstd", "dwc", "dbc"), leaves):
        out[name] = torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
    return out


def masked_mean(x, mask):
    if mask is None:
        return x.mean()
    w = mask.to(x.dtype)
    return (x * w).sum() / w.sum()


def ppo_loss_ref(logp, old_logp, adv, value, old_value, ret, entropy, clip, value_coef, entropy_coef, clipped_value=True, mask=None,
                 dtype=torch.float64):
    """-> (loss, action_loss, value_loss, clip_frac, approx_kl), 0-dim; rows [B]."""
    c = lambda t: t.to(dtype).reshape(-1)      # noqa: E731
    logp, old_logp, adv, value, old_value, ret = c(logp), c(old_logp), c(adv), c(value), c(old_value), c(ret)
    clip, value_coef, entropy_coef = f32_scalar(clip), f32_scalar(value_coef), f32_scalar(entropy_coef)
    ratio = torch.exp(logp - old_logp)
    s1 = ratio * adv
    s2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
    action_loss = -masked_mean(torch.min(s1, s2), mask)
    if clipped_value:
        vc = old_value + torch.clamp(value - old_value, -clip, clip)
        value_loss = 0.5 * masked_mean(torch.max((value - ret) ** 2, (vc - ret) ** 2), mask)
    else:
        value_loss = 0.5 * masked_mean((ret - value) ** 2, mask)
    loss = value_coef * value_loss + action_loss - entropy_coef * entropy.to(dtype).reshape(())
    with torch.no_grad():
        clip_frac = masked_mean(((ratio - 1.0).abs() > clip).to(dtype), mask)
        approx_kl = masked_mean(old_logp - logp, mask)
    return loss, action_loss, value_loss, clip_frac, approx_kl


PPO_OUT = ("loss", "action_loss", "value_loss", "clip_frac", "approx_kl")


def ppo_loss_run(rows, entropy, hyper, clipped_value, mask, dtype, dloss=1.0):
    """Forward + backward in `dtype` from float32 `rows` = (logp, old_logp, adv, value, old_value, ret) and `hyper` = (clip,
    value_coef, entropy_coef).  -> dict of the five outputs and dlogp, dvalue, dentropy."""
    logp, old_logp, adv, value, old_value, ret = (t.detach().to(dtype) for t in rows)
    logp.requires_grad_(True)
    value.requires_grad_(True)
    ent = entropy.detach().to(dtype).requires_grad_(True)
    outs = ppo_loss_ref(logp, old_logp, adv, value, old_value, ret, ent, *hyper, clipped_value=clipped_value, mask=mask, dtype=dtype)
    (outs[0] * dloss).backward()
    res = {k: v.detach() for k, v in zip(PPO_OUT, outs)}
    res.update(dlogp=logp.grad, dvalue=value.grad, dentropy=ent.grad)
    return res


def bar_of(ref64, stock32):
    """(bar, e32): the rule of the module docstring for one quantity (tensors of any one shape; finite)."""
    ref64 = ref64.detach().double().cpu()
    e32 = float((stock32.detach().double().cpu() - ref64).abs().max()) if ref64.numel() else 0.0
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    return max(4.0 * e32, 1e-6 * scale), e32


def err_of(got, ref64):
    return float((got.detach().double().cpu() - ref64.detach().double().cpu()).abs().max()) if ref64.numel() else 0.0


def check(tag, got, ref64, stock32, log=None):
    """Print the figures of one compared quantity, then assert it is inside its bar.  NaNs must sit where the oracle's do; the
    bar is taken over the finite entries."""
    g, r, s = got.detach().double().cpu().reshape(-1), ref64.detach().double().reshape(-1), stock32.detach().double().reshape(-1)
    assert g.shape == r.shape, (tag, tuple(got.shape), tuple(ref64.shape))
    nan = torch.isnan(r)
    assert torch.equal(torch.isnan(g), nan), f"{tag}: NaN where the oracle has none, or none where it has"
    ok = ~nan
    bar, e32 = bar_of(r[ok], s[ok])
    e = err_of(g[ok], r[ok])
    line = f"{tag}: error {e:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}  max|ref| {float(r[ok].abs().max()) if ok.any() else math.nan:.3e}"
    print(line)
    if log is not None:
        log.append(line)
    assert e <= bar, line
    return e, e32, bar


# ----------------------------------------------------------------------------- inputs
def eval_inputs(B, K, A, logstd="small", far=False, seed=0):
    """(x [B,K], wm [A,K], bm [A], logstd [A,1], wc [1,K], bc [1], action [B,A]) float32 on the CPU, and upstream gradients (g value
    [B,1], g logp [B], g entropy 0-dim).  logstd: "small" (|.| <= 0.5) or "pm3" (+3, -3, +3, ...); far: actions exactly 5 sigma
    from the float32 mean, alternating sides, else about one sigma."""
    g = torch.Generator(); g.manual_seed(1000 * B + 10 * K + A + 7919 * seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1      # noqa: E731
    x = torch.randn(B, K, generator=g)
    wm, bm = u(A, K) / K ** 0.5, u(A) / K ** 0.5
    wc, bc = u(1, K) / K ** 0.5, u(1) / K ** 0.5
    ls = 0.5 * u(A, 1) if logstd == "small" else torch.tensor([3.0 if a % 2 == 0 else -3.0 for a in range(A)]).view(A, 1)
    mean = F.linear(x, wm, bm)
    z = torch.randn(B, A, generator=g)
    if far:
        z = torch.tensor([[5.0 if (b + a) % 2 == 0 else -5.0 for a in range(A)] for b in range(B)])
    action = mean + z * ls.t().exp()
    grads = (torch.rand(B, 1, generator=g) + 0.5, torch.rand(B, generator=g) + 0.5, torch.tensor(0.75))
    return (x, wm, bm, ls, wc, bc, action), grads


CLIP, VALUE_COEF, ENTROPY_COEF = 0.2, 0.5, 0.01
# one row per combination: (log ratio, sign of adv, value - old_value, returns - old_value).  Ratios 0.55-0.67 / 0.86-1.16 / 1.49-1.82
# and exactly 1 against the clip range [0.8, 1.2]; value steps inside (0.1) and outside (0.5) the clip of 0.2; returns far to
# either side, so that the unclipped and the clipped squared error each win the maximum (never a tie, never a clamp edge)
_LOG_RATIO = (-0.5, -0.1, 0.0, 0.1, 0.5)
_ADV_SIGN = (1.0, -1.0, 0.0)
_VSTEP = (-0.5, -0.1, 0.1, 0.5)
_RET = (-1.0, 1.0)
PPO_PATTERN = [(lr, sa, vs, rt) for rt in _RET for vs in _VSTEP for sa in _ADV_SIGN for lr in _LOG_RATIO]     # 120 rows


def ppo_inputs(B, seed=0):
    """rows (logp, old_logp, adv, value, old_value, ret) [B] float32 + entropy [1]: row i sits on the branch combination
    PPO_PATTERN[(i + B) % 120], with seeded magnitudes that keep it there."""
    g = torch.Generator(); g.manual_seed(31 * B + seed)
    r = lambda: torch.rand(B, generator=g)      # noqa: E731
    pat = torch.tensor([PPO_PATTERN[(i + B) % len(PPO_PATTERN)] for i in range(B)], dtype=torch.float32).view(B, 4)
    old_logp = -1.0 - 2.0 * r()
    jitter = torch.where(pat[:, 0] == 0, torch.zeros(B), (r() - 0.5) * 0.1 * (1 + (pat[:, 0].abs() > 0.3).float()))
    logp = torch.where(pat[:, 0] == 0, old_logp, old_logp + pat[:, 0] + jitter)     # exactly old_logp where the ratio is to be 1
    adv = pat[:, 1] * (0.25 + 1.5 * r())
    old_value = 2.0 * r() - 1.0
    value = old_value + pat[:, 2] * (0.8 + 0.4 * r())        # 0.08-0.12 inside, 0.4-0.6 outside the clip of 0.2
    ret = old_value + pat[:, 3] * (1.0 + 0.5 * r())
    entropy = torch.tensor([1.3 + 0.1 * seed])
    return (logp, old_logp, adv, value, old_value, ret), entropy
