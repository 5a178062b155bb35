"""The model of tests/tree_oracle.py under the rule of ngw_tree_set_rule (include/ngw.h): rows by the spread rule, a discounted backup.  Both are
written out here in plain Python integers and np.float32 on the model's dict - not through tree.py's references (tests/test_tree_rule_cpu.py
holds the two to each other)."""
import numpy as np

import tree_oracle as TM

F32 = np.float32
LO, HI = F32(2.0 ** -64), F32(2.0 ** 64)


def wrap64(x):
    x &= 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >> 63 else x


def discounted(x, g):
    """D(x): x for g = 65536, else the int64 product g * x, wrapped, shifted right by 16 arithmetically."""
    return x if g == 65536 else wrap64(g * x) >> 16


def returns_to_go(rewards, n, boot, g):
    """G_0 .. G_n of one pair: rewards a list of T ints, n executed steps, G_n = boot + the rewards behind the executed steps."""
    G = [0] * n + [boot + sum(rewards[n:])]
    for t in range(n - 1, -1, -1):
        G[t] = wrap64(rewards[t] + discounted(G[t + 1], g))
    return G


def spread_row(n, w, mask, c, q_init, spread, p=None):
    """One row by the spread rule -> (float32 [A], bad).  n, w: the visits and returns of the node; p: its priors or None."""
    A = len(n)
    bad = False
    with np.errstate(all='ignore'):
        q, cp = [], []
        for a in range(A):
            pa = F32(1)
            if p is not None:
                x = F32(p[a])
                bad = bad or not (x >= 0 and x <= HI)
                pa = x if (x >= LO and x <= HI) else F32(0)
            q.append(F32(int(w[a])) / F32(int(n[a])) if n[a] > 0 else F32(q_init))
            cp.append(F32(F32(c) * pa))
        k = [0] * A
        total = sum(int(x) for x in n)
        if int(mask):
            for i in range(spread):
                root = F32(np.sqrt(F32(total + 1 + i)))
                pick, best = -1, None
                for a in range(A):
                    if not (int(mask) >> a) & 1:
                        continue
                    s = F32(q[a] + F32(F32(cp[a] * root) / F32(1 + int(n[a]) + k[a])))
                    if pick < 0 or s > best:
                        pick, best = a, s
                k[pick] += 1
    return np.array(k, F32), bad


class RuleModel(TM.TreeModel):
    """TreeModel with spread = S and discount_q16 = g."""

    def __init__(self, *args, spread=1, discount_q16=65536, **kw):
        self.spread, self.g = int(spread), int(discount_q16)
        super().__init__(*args, **kw)

    def reweight(self, keys):
        for k in keys:
            nd = self.node[k]
            nd.row, bad = spread_row(nd.n, nd.w, nd.mask, self.c, self.q_init, self.spread, None if self.priors is None else nd.p)
            self.bad = self.bad or bad

    def iterate(self, e, bootstrap=None, grow=True):
        """TreeModel.iterate with rule 4's G_t replaced by the discounted one."""
        depth, length, count = e['depth'], e['length'], len(e['depth'])
        T = e['rewards'].shape[0]
        leaf = [0] * count
        for j in range(count):
            d = int(depth[j])
            if grow and 1 <= d < int(length[j]):
                leaf[j] = int(e['keys'][d - 1, j])
        held, grown = self.insert(leaf)
        for j in range(count):
            if held[j]:
                self.node[leaf[j]].mask = np.uint64(e['masks'][int(depth[j]), j])
        touched, backed = set(), 0
        for j in range(count):
            d = int(depth[j])
            if d < 1:
                continue
            n = min(max(int(length[j]), 0), T)
            G = returns_to_go([int(x) for x in e['rewards'][:, j]], n, 0 if bootstrap is None else int(bootstrap[j]), self.g)
            for t in range(min(d, n - 1), -1, -1):
                k = int(e['before'][t, j]) if t < d else (leaf[j] if held[j] else 0)
                if not k:
                    continue
                nd, a = self.node[k], int(e['actions'][t, j])
                nd.n[a] += 1
                nd.w[a] += G[t]
                touched.add(k)
                backed += 1
        self.reweight(sorted(touched | {leaf[j] for j in range(count) if held[j]}))
        self.report.append((int((length >= 1).sum()), grown, sum(1 for j in range(count) if leaf[j] and not held[j]), backed, int(depth.max()) if count else 0))
        e['leaf'], e['held'] = np.array(leaf, np.uint64), np.array(held, bool)
        self.last = e
        self.it += 1
