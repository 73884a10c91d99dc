"""What the GPU tests of the public surface (test_gpu_policy.py, test_gpu_evaluate.py, test_gpu_loss.py) build
alike: a small env, a DevicePolicy of the reference's default sizes on it, and a replay buffer of collect
steps."""
import gnn_model as gm
import policy_model as pm
from lsm import gnn, policy

DEV = "cuda:0"


def heads(env, recurrent_N=1, seed=0):
    """(DevicePolicy, the two head configs and state dicts) for env: the reference's default sizes."""
    N, OBS, F = env.N, env.OBS, env.F
    acfg, ccfg = gnn.GnnConfig(F=F, aggr="node"), gnn.GnnConfig(F=F, aggr="global_mean")
    ah = policy.HeadConfig(kind="actor", in0=OBS, in1=16, num_actions=25, recurrent_N=recurrent_N)
    ch = policy.HeadConfig(kind="critic", in0=N * OBS, in1=16, recurrent_N=recurrent_N)
    asd, csd = pm.random_head_weights(ah, 11 + seed), pm.random_head_weights(ch, 12 + seed)
    pol = policy.DevicePolicy(gnn.GraphEncoder(acfg, gm.default_weights(acfg, 5)[1], DEV),
                              policy.PolicyHead(ah, policy.pack_head_weights(asd, ah), DEV),
                              gnn.GraphEncoder(ccfg, gm.default_weights(ccfg, 6)[1], DEV),
                              policy.PolicyHead(ch, policy.pack_head_weights(csd, ch), DEV))
    return pol, (ah, asd), (ch, csd)


def env(layout="reference"):
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    return GpuGraphVecEnv(EnvArgs(num_agents=3, seed=1), num_envs=4, device=DEV, return_numpy=False, build_infos=False,
                          adj_layout=layout)


def collect(env, pol, T):
    """T collect steps into a DeviceGraphBuffer with policy rows."""
    import torch
    from lsm.buffer import DeviceGraphBuffer
    buf = DeviceGraphBuffer(env, episode_length=T, policy_rows=dict(hidden_size=64, recurrent_N=1, act_dim=1,
                                                                    num_actions=None))
    buf.warmup(0)
    g = torch.Generator(device=DEV).manual_seed(5)
    for t in range(T):
        out = pol.get_actions(env, buf.rnn_states[t], buf.rnn_states_critic[t], buf.masks[t], generator=g, buffer=buf)
        buf.insert_step(out["actions_env"], 0, value_preds=out["values"],
                        policy={k: out[k] for k in ("actions", "action_log_probs", "rnn_states", "rnn_states_critic")})
    return buf
