"""The weighted choice among valid actions on the host: the public contract of include/ngw.h (ngw_sample_actions) in numpy - the counterpart
of playout.choose_actions, whose Philox and k-th-set-bit it reuses.  A host that knows a pair's valid-action mask word and its weights
computes here the action and the mass the device returned for it, bit for bit:

    m = the mask word; all n_actions bits where it is 0
    w = word (t & 3) of Philox4x32-10, counter (t >> 2, 0, lo32(p), hi32(p)), key (lo32(seed), hi32(seed) ^ SAMPLE_TAG)
    v[a] = x[a] where bit a of m is set and 2^-64 <= x[a] <= 2^64, else +0      (negative, NaN, above 2^64: F_BAD_WEIGHT)
    c[a] = c[a-1] + v[a] in float32, one add per action;  mass = c[n_actions - 1]
    mass > 0:  u = float32(w >> 8) * 2^-24, thr = u * mass, the smallest a with v[a] > 0 and c[a] > thr
    mass == 0: k = (w * popcount(m)) >> 32, the (k + 1)-th set bit of m

p is the pair's global number (first_pair + its position in the call).  Nothing here touches the device."""
import collections

import numpy as np

from .playout import _LO, _S32, kth_set_bit, philox4x32_10

SAMPLE_TAG = 0x53414D50           # include/ngw.h NGW_SAMPLE_TAG
WEIGHT_MIN, WEIGHT_MAX = np.float32(2.0 ** -64), np.float32(2.0 ** 64)


class Sampled(collections.namedtuple('Sampled', 'action mass mask_words')):
    """What sample_actions() / step_sampled() return: 'action' int32, 'mass' float32 (the sum of the valid actions' cleaned weights: log pi(a)
    = log weights[a] - log mass; 0 where the uniform rule chose) and 'mask_words' uint64 (the valid-action word the choice was made under,
    all n_actions bits where no action was valid; what a learner stores to recompute masked log-probabilities), each [count].  numpy arrays,
    or torch tensors (the words int64 there, the same bits).  A named tuple whose fields can also be read by name: s['mass']."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)


def words_of(tag, seed, pairs, t):
    """w of the contract under `tag` for the global pair numbers `pairs` (uint64 values, any shape) at step number t (an int, or an array
    broadcastable against pairs) -> uint32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    p = np.asarray(pairs).astype(np.uint64)
    t = np.asarray(t, np.int64)
    if (t < 0).any():
        raise ValueError("t: steps are numbered from 0")
    p, t = np.broadcast_arrays(p, t)
    zero = np.zeros(p.shape, np.uint64)
    words = philox4x32_10(((t >> 2).astype(np.uint64), zero, p & _LO, p >> _S32), (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) ^ tag)))
    return np.choose(t & 3, words)


def sample_words(seed, pairs, t):
    """w of ngw_sample_actions for the global pair numbers `pairs` at step number t -> uint32."""
    return words_of(SAMPLE_TAG, seed, pairs, t)


def bad_weights(weights):
    """Does any weight raise F_BAD_WEIGHT: negative, NaN or above 2^64 (infinity included)?  -0.0 is zero."""
    x = np.asarray(weights, np.float32)
    with np.errstate(invalid='ignore'):
        return bool((~((x >= 0) & (x <= WEIGHT_MAX))).any())


def choose_weighted(mask_words, weights, seed, pairs, t, n_actions, words=None):
    """The choice of the contract for each pair: mask_words = the uint64 valid-action words of the pairs' states, [count] (int64 words over the
    same bits are taken too), weights = float32 [count, n_actions] (or [n_actions], the same for every pair), pairs = their global pair
    numbers, t = the step number (an int or an array), n_actions = the length of the action list.  words: the Philox words to use in the
    place of sample_words(seed, pairs, t) - a weighted playout passes its own stream's (playout.playout_words).
    -> (action int32 [count], mass float32 [count], m uint64 [count]: the word the choice was made under)."""
    n_actions = int(n_actions)
    if not 1 <= n_actions <= 48:
        raise ValueError("n_actions: %d outside [1, 48]" % n_actions)
    m = np.asarray(mask_words)
    m = (m.view(np.uint64) if m.dtype == np.int64 else m.astype(np.uint64)).reshape(-1)
    every = np.uint64((1 << n_actions) - 1)
    if (m & ~every).any():
        raise ValueError("mask_words: a bit at or above n_actions = %d is set" % n_actions)
    x = np.asarray(weights)
    if x.dtype != np.float32 or x.shape not in ((n_actions,), (m.size, n_actions)):
        raise ValueError("weights: float32 [%d, %d] or [%d] expected, got %s %s" % (m.size, n_actions, n_actions, x.dtype, x.shape))
    x = np.broadcast_to(x, (m.size, n_actions))
    m = np.where(m == 0, every, m)
    w = np.broadcast_to(sample_words(seed, pairs, t) if words is None else np.asarray(words, np.uint32), m.shape)
    zero = np.float32(0)
    c = np.zeros(m.size, np.float32)
    cs, vs = [], []
    with np.errstate(invalid='ignore'):
        for a in range(n_actions):                     # one float32 add per action, in action order
            xa = x[:, a]
            keep = (((m >> np.uint64(a)) & np.uint64(1)) != 0) & (xa >= WEIGHT_MIN) & (xa <= WEIGHT_MAX)
            v = np.where(keep, xa, zero).astype(np.float32)
            c = (c + v).astype(np.float32)
            vs.append(v); cs.append(c)
    mass = c
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    thr = (u * mass).astype(np.float32)
    pick = np.full(m.size, -1, np.int32)
    last = np.full(m.size, -1, np.int32)
    for a in range(n_actions):
        pos = vs[a] > zero
        pick = np.where(pos & (cs[a] > thr) & (pick < 0), np.int32(a), pick)
        last = np.where(pos, np.int32(a), last)
    weighted = np.where(pick < 0, last, pick)
    n = ((m[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).sum(-1).astype(np.uint64)
    uniform = kth_set_bit(m, (w.astype(np.uint64) * n) >> _S32)
    return np.where(mass > zero, weighted, uniform).astype(np.int32), mass, m


def check_weights(weights, count, n_actions, dev, per_pair=True):
    """The weights argument of a sampling call -> (a float32 device tensor, action-major [n_actions, count] - or [n_actions] where not
    per_pair -, whether it was uploaded here).  A torch tensor must be float32, contiguous, on `dev` and of exactly that shape: it is used in
    place.  Anything else is taken as a host array [count, n_actions] ([n_actions]) of real numbers, rounded to float32, transposed and
    uploaded.  Values are never refused here: the device reports a bad one through F_BAD_WEIGHT, for host and device inputs alike."""
    import torch
    shape = (n_actions, count) if per_pair else (n_actions,)
    if isinstance(weights, torch.Tensor):
        if weights.dtype != torch.float32 or tuple(weights.shape) != shape or not weights.is_contiguous() or weights.device != dev:
            raise ValueError("weights: a contiguous float32 tensor %s on %s expected (action-major), got %s %s on %s" % (
                list(shape), dev, weights.dtype, list(weights.shape), weights.device))
        return weights, False
    x = np.asarray(weights)
    if x.dtype.kind not in 'fiu' or x.dtype == np.float16:
        raise ValueError("weights: float32 numbers expected, got dtype %s" % x.dtype)
    host_shape = (count, n_actions) if per_pair else (n_actions,)
    if x.shape != host_shape:
        raise ValueError("weights: an array of shape %s expected (one row per state, one column per action), got %s" % (list(host_shape), list(x.shape)))
    with np.errstate(over='ignore', invalid='ignore'):
        x = np.ascontiguousarray(x.astype(np.float32).T if per_pair else x.astype(np.float32))
    return torch.from_numpy(x).to(dev), True


def check_seed(seed, first_pair, t):
    seed, first_pair, t = int(seed), int(first_pair), int(t)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed: %d outside [0, 2^64)" % seed)
    if not 0 <= first_pair < 1 << 64:
        raise ValueError("first_pair: %d outside [0, 2^64)" % first_pair)
    if not 0 <= t < 1 << 32:
        raise ValueError("t: %d outside [0, 2^32)" % t)
    return seed, first_pair, t


def sample_call(env, holder, src, idx, limit, name, weights, seed, first_pair, t, device):
    """The one launch behind VecNovelGridworld.sample_actions and Snapshot.sample_actions: src = a snapshot's C handle (None: the envs' current
    states), idx = the rows (None, a checked list or a device tensor: snapshot.index_arg); `holder` keeps what was uploaded alive.
    -> Sampled of [count] fields."""
    import ctypes as C

    import torch

    from . import _cabi
    from .snapshot import enqueue_ordered, index_arg
    seed, first_pair, t = check_seed(seed, first_pair, t)
    ptr, count, dev, uploaded = index_arg(env, idx, limit, name)
    wt, mine = check_weights(weights, count, env.n_actions, dev)
    if mine:
        uploaded = uploaded + [wt]                     # (a caller's own tensor is the caller's to keep, as an index tensor is)
    action = torch.full((count,), -1, dtype=torch.int32, device=dev)
    mass = torch.zeros(count, dtype=torch.float32, device=dev)
    words = torch.zeros(count, dtype=torch.int64, device=dev)
    enqueue_ordered(env, holder, lambda: _cabi.lib().ngw_sample_actions(
        env._h, src, ptr, count, C.c_void_p(wt.data_ptr()), count, seed, first_pair, t, C.c_void_p(action.data_ptr()), C.c_void_p(mass.data_ptr()),
        C.c_void_p(words.data_ptr())), count, uploaded, device)
    if device:
        return Sampled(action, mass, words)
    return Sampled(action.cpu().numpy(), mass.cpu().numpy(), words.cpu().numpy().view(np.uint64))
