"""Numpy model of the recurrent-policy hand-off (include/lsm_recurrent.h): the chunk addressing of
GraphReplayBuffer.recurrent_generator on [T][M][row] buffers, the three field kinds of the chunk gather
and the per-step row copies. The model and the fixtures recorded from the reference
(tests/golden/recurrent/) check each other; the HIP code is then compared with both."""
import numpy as np

import returns_model as rm

# GraphReplayBuffer.recurrent_generator's yield order (graph_buffer.py:751-755)
NAMES = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic",
         "actions", "value_preds", "returns", "masks", "active_masks", "action_log_probs", "advantages",
         "available_actions")
FIRST = ("rnn_states", "rnn_states_critic")
POLICY = ("rnn_states", "rnn_states_critic", "actions", "action_log_probs", "available_actions")


def data_chunks(L, T, M):
    return (T * M) // L


def chunk_rows(chunks, L, T, M):
    """Flat source rows of a minibatch in destination order: entry l * C + b is the buffer row
    (f % T) * M + f // T of sample f = chunks[b] * L + l; -1 for a chunk id outside [0, data_chunks)."""
    c = np.asarray(chunks, dtype=object)   # Python integers: ids like 2**40 * L must not wrap
    ok = np.array([0 <= int(x) < data_chunks(L, T, M) for x in c], dtype=bool)
    c = np.where(ok, c, 0).astype(np.int64)
    f = c[None, :] * L + np.arange(L, dtype=np.int64)[:, None]          # [L, C]
    rows = (f % T) * M + f // T
    return np.where(ok[None, :], rows, -1).reshape(-1)


def first_rows(chunks, L, T, M):
    """Source rows of the recurrent states: step 0 of every chunk."""
    return chunk_rows(chunks, L, T, M)[:len(chunks)]


def cast_view(x, T, M):
    """The reference's _cast / transpose(1, 2, 0, ...) view of a [T * M, ...] array of buffer rows."""
    x = np.asarray(x)
    return x.reshape((T, M) + x.shape[1:]).swapaxes(0, 1).reshape((T * M,) + x.shape[1:])


def gather_rows(src, chunks, L, T, M):
    return rm.gather_rows(src, chunk_rows(chunks, L, T, M))


def gather_first(src, chunks, L, T, M):
    return rm.gather_rows(src, first_rows(chunks, L, T, M))


def gather_compact_adj(A, masks, chunks, L, T, M, N):
    return rm.gather_compact_adj(A, masks, chunk_rows(chunks, L, T, M), N)


def pack_bits(bits):
    """[rows, E] bool -> [rows, W] uint64 disconnect words."""
    rows, E = bits.shape
    m = np.zeros((rows, (E + 63) // 64), dtype=np.uint64)
    for e in range(E):
        m[:, e // 64] |= bits[:, e].astype(np.uint64) << np.uint64(e % 64)
    return m


def copy_rows(src, dones, zero_on_done):
    """dst[m] = 0 where zero_on_done and dones[m] != 0, else src[m]."""
    out = np.array(src, copy=True)
    if zero_on_done:
        out[np.asarray(dones).reshape(-1) != 0] = 0
    return out
