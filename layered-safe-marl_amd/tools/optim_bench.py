"""Device time of the end of a PPO update -- the gradient norm, the clipping and Adam's step of both networks --
at the reference's default network sizes (3 agents):

  (A) fused          lsm.policy.DevicePolicy.optimizer_step: one lsm_optim_step call (csrc/lsm_optim.hip), three
                     launches for the actor's and the critic's group together, on the blobs and on the gradients
                     the backward passes left, weights updated in place;
  (B) torch_bare     clip_grad_norm_ + torch.optim.Adam.step() of two optimisers (torch's default foreach path) on
                     device parameters of the same shapes that already hold .grad: torch's cost without any
                     hand-over;
  (C) torch_recipe   what a learner on this project paid before: every gradient view cloned into .grad, (B), and
                     GraphEncoder.load / PolicyHead.load of all four modules from the state dicts (pack on the host,
                     upload), which synchronises.

Method: (A) is checked first against tests-style arithmetic -- one step of (B) from the same weights and gradients,
the same step in float64 as the truth, tools/bench_common.py's criterion on every parameter. Then a warm-up, HIP
events around `reps` back-to-back calls, the sides in alternating rounds, and the median / min / max of the rounds'
means (alternated()). (C) contains host work; the events span it because the next call's device work waits for it.
No ratio is asserted: the figures are recorded as found.

    python layered-safe-marl_amd/tools/optim_bench.py [--out FILE] [--quick]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_common import alternated, criterion, emit  # noqa: E402
from gnn_bench import seeded_state_dict  # noqa: E402
from policy_bench import seeded_state_dict as head_state_dict  # noqa: E402

DEV = "cuda:0"
PROFILE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "optim_bench.json")
LAUNCHES = 3   # include/lsm_optim.h: partial sums, finalise, apply -- whatever the number of groups


def build():
    """A DevicePolicy of the reference's default sizes with a gradient in every module, the two DeviceAdam, and
    per network the torch parameters {state-dict name: Parameter} (encoder names under 'gnn.')."""
    import torch
    from lsm import gnn, optim, policy
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    env = GpuGraphVecEnv(EnvArgs(num_agents=3, seed=1), num_envs=4, device=DEV, return_numpy=False, build_infos=False)
    env.reset(0)
    N, OBS, F, E = env.N, env.OBS, env.F, env.E
    acfg, ccfg = gnn.GnnConfig(F=F, aggr="node"), gnn.GnnConfig(F=F, aggr="global_mean")
    ah = policy.HeadConfig(kind="actor", in0=OBS, in1=16, num_actions=25)
    ch = policy.HeadConfig(kind="critic", in0=N * OBS, in1=16)
    sds = {"actor": (seeded_state_dict(acfg), head_state_dict(ah, 1)), "critic": (seeded_state_dict(ccfg), head_state_dict(ch, 2))}
    pol = policy.DevicePolicy(gnn.GraphEncoder(acfg, gnn.pack_weights(sds["actor"][0], acfg, prefix=""), DEV),
                              policy.PolicyHead(ah, policy.pack_head_weights(sds["actor"][1], ah), DEV),
                              gnn.GraphEncoder(ccfg, gnn.pack_weights(sds["critic"][0], ccfg, prefix=""), DEV),
                              policy.PolicyHead(ch, policy.pack_head_weights(sds["critic"][1], ch), DEV))
    g = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *s: torch.randn(s, generator=g, device=DEV)
    B = 4 * N
    node, adj = env.t_node.view(B, E, F), env.reference_adj().reshape(B, E, E).contiguous()
    masks = torch.ones(B, 1, device=DEV)
    for enc in (pol.actor_encoder, pol.critic_encoder):
        enc.backward(node, adj, rnd(B, 16), env.agent_id.reshape(-1), embed=True)
    pol.actor_head.backward(rnd(B, OBS), rnd(B, 16), rnd(B // 3, 1, 64), masks, 3, dlogits=0.01 * rnd(B, 25))
    pol.critic_head.backward(rnd(B, N * OBS), rnd(B, 16), rnd(B // 3, 1, 64), masks, 3, dvalues=rnd(B, 1))
    cfg = optim.AdamConfig(lr=7e-4)
    opts = {"actor": optim.DeviceAdam(cfg, [pol.actor_encoder, pol.actor_head], DEV),
            "critic": optim.DeviceAdam(cfg, [pol.critic_encoder, pol.critic_head], DEV)}
    env.close()
    return pol, opts


def named(pol, who, what):
    """{name: tensor} over a network's two modules: what = 'weights' (copies of the blob's entries) or 'grads'
    (views of the last backward's)."""
    enc, head = (pol.actor_encoder, pol.actor_head) if who == "actor" else (pol.critic_encoder, pol.critic_head)
    if what == "grads":
        return dict(enc.gradients(), **head.gradients())
    return {k: v.to(DEV) for k, v in dict(enc.state_dict(), **head.state_dict()).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PROFILE)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    ap.add_argument("--record-only", action="store_true", help="record the criterion's figures without ending the run on a miss")
    a = ap.parse_args()
    import torch
    pol, opts = build()
    whos = ("actor", "critic")
    grads = {w: named(pol, w, "grads") for w in whos}
    w0 = {w: named(pol, w, "weights") for w in whos}

    def torch_side(dtype):
        params = {w: {k: torch.nn.Parameter(v.to(dtype).clone()) for k, v in w0[w].items()} for w in whos}
        adam = {w: torch.optim.Adam(params[w].values(), lr=7e-4, eps=1e-5, weight_decay=0.0) for w in whos}
        return params, adam

    def set_grads(params, dtype):
        for w in whos:
            for k, p in params[w].items():
                p.grad = grads[w][k].to(dtype).clone()

    def clip_and_step(params, adam):
        for w in whos:
            torch.nn.utils.clip_grad_norm_(params[w].values(), 10.0)
            adam[w].step()

    # the check: one step of all three from the same weights and gradients
    checks = {}
    p64, a64 = torch_side(torch.float64)
    p32, a32 = torch_side(torch.float32)
    for p, ad, dt in ((p64, a64, torch.float64), (p32, a32, torch.float32)):
        set_grads(p, dt)
        clip_and_step(p, ad)
    res = pol.optimizer_step(opts["actor"], opts["critic"])
    for w in whos:
        fused = named(pol, w, "weights")
        chk = criterion(fused, {k: v.detach() for k, v in p32[w].items()}, {k: v.detach() for k, v in p64[w].items()},
                        list(fused), w, bound="4 * e32 + 4 ulp =", enforce=not a.record_only)
        worst = max(chk, key=lambda n: chk[n]["fused_err_vs_float64"] / max(chk[n]["tolerance"], 1e-300))
        checks[w] = {"worst_tensor": worst, "worst_check": chk[worst], "grad_norm": float(res[w]["grad_norm"]),
                     "clip_coef": float(res[w]["clip_coef"]), "parameters": len(fused),
                     "floats": int(sum(v.numel() for v in fused.values()))}

    # the timed sides
    params, adam = torch_side(torch.float32)
    set_grads(params, torch.float32)
    mods = {"actor": (pol.actor_encoder, pol.actor_head), "critic": (pol.critic_encoder, pol.critic_head)}

    def recipe():
        for w in whos:
            for k, p in params[w].items():
                p.grad = grads[w][k].clone()
        clip_and_step(params, adam)
        for w in whos:
            sd = {k: p.detach() for k, p in params[w].items()}
            mods[w][0].load(sd)
            mods[w][1].load(sd)

    sides = {"fused": (lambda: pol.optimizer_step(opts["actor"], opts["critic"]), 20 if a.quick else 100),
             "torch_bare": (lambda: clip_and_step(params, adam), 5 if a.quick else 20),
             "torch_recipe": (recipe, 3 if a.quick else 10)}
    for fn, _ in sides.values():   # warm-up
        fn()
    t = alternated(sides)
    out = dict(t, checks=checks, launches_fused=LAUNCHES, groups=2,
               ratio_torch_bare_over_fused=t["torch_bare"]["median"] / t["fused"]["median"],
               ratio_torch_recipe_over_fused=t["torch_recipe"]["median"] / t["fused"]["median"])
    print("optimizer_step %.4f ms [%.4f, %.4f]; torch clip + Adam on .grad %.4f ms (x%.2f); with the .grad copies and "
          "four load() %.4f ms (x%.2f)" % (t["fused"]["median"], t["fused"]["min"], t["fused"]["max"],
                                          t["torch_bare"]["median"], out["ratio_torch_bare_over_fused"],
                                          t["torch_recipe"]["median"], out["ratio_torch_recipe_over_fused"]),
          file=sys.stderr, flush=True)
    emit({"optim_bench": out}, a.out)


if __name__ == "__main__":
    main()
