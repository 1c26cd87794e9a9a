"""NumPy restatement of the reference's L-BFGS operators (pykrylov/linop/lbfgs.py) with a pluggable inner product.
TEST INFRASTRUCTURE ONLY.

With ``dot=np.dot`` it repeats the reference's arithmetic call for call (same operands, same operand order, the same
strided column views, so BLAS sums in the same order): tests/golden/lbfgs.npz, written by the reference itself, is
reproduced bit for bit.  With ``dot=oracle.gpu_order.stream_dot`` every inner product is summed in the order of the
device's streaming dot, and the device operators must reproduce the result bit for bit -- everything else (one rounding
per multiply, add and divide) is the same arithmetic on both sides.
"""
import numpy as np

SCENARIOS = ("none", "few", "full", "wrap", "reject", "restart")
# op codes of a scenario: (code, pool index)
STORE, STORE_NEG, STORE_ZERO, RESTART = 0, 1, 2, 3
POOL = 12          # pairs a scenario may draw from (npairs + 2 <= POOL for every npairs tested: 1, 5, 8)


def make_pairs(n, count, seed):
    """`count` secant pairs y = s o (1 + u) + 0.01 g with seeded s, g normal and u uniform: s'y > 0, and B (H v) = v to
    about 2e-16 in the relative 2-norm.  Returns (S, Y) of shape (count, n)."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((count, n))
    U = rng.random((count, n))
    G = rng.standard_normal((count, n))
    return S, S * (1.0 + U) + 0.01 * G


def scenario_ops(name, npairs):
    """The (code, pool index) steps of a scenario for a ring of `npairs` slots."""
    st = lambda k: [(STORE, i) for i in range(k)]     # noqa: E731
    if name == "none":
        return []
    if name == "few":                                  # fewer than npairs (none when npairs == 1)
        return st(max(0, min(npairs - 1, 3)))
    if name == "full":
        return st(npairs)
    if name == "wrap":
        return st(npairs + 2)
    if name == "reject":                               # rejected pairs in the middle: y = -s, y = 0
        k = max(1, npairs // 2)
        return st(k) + [(STORE_NEG, k), (STORE_ZERO, k + 1)] + [(STORE, i) for i in range(k, npairs + 1)]
    if name == "restart":                              # a restart followed by two stores
        return st(min(npairs, 3)) + [(RESTART, 0), (STORE, 3), (STORE, 4)]
    raise KeyError(name)


def replay(target, ops, S, Y):
    """Run the steps on anything with store(s, y) / restart() (the reference, the restatement, the device operators)."""
    for code, i in ops:
        if code == STORE:
            target.store(S[i], Y[i])
        elif code == STORE_NEG:
            target.store(S[i], -S[i])
        elif code == STORE_ZERO:
            target.store(S[i], np.zeros_like(S[i]))
        else:
            target.restart()


class RefLBFGS(object):
    """State and products of lbfgs.py's InverseLBFGSOperator (`inverse`) and CompactLBFGSOperator (`compact`)."""

    def __init__(self, n, npairs=5, scaling=False, dot=np.dot):
        self.n, self.npairs, self.scaling, self.dot = n, npairs, scaling, dot
        self.insert = 0                                           # lbfgs.py:48
        self.accept_threshold = 1.0e-20                           # :51
        self.s = np.zeros((n, npairs), 'd')                       # :54-55 (np.empty there)
        self.y = np.zeros((n, npairs), 'd')
        self.alpha = np.empty(npairs, 'd')                        # :57
        self.ys = [None] * npairs                                 # :58
        self.gamma = 1.0                                          # :59

    def store(self, new_s, new_y):                                # lbfgs.py:70-87
        ys = self.dot(new_s, new_y)                               # :77
        if ys <= self.accept_threshold:                           # :78
            return False
        insert = self.insert
        self.s[:, insert] = new_s.copy()                          # :83-84
        self.y[:, insert] = new_y.copy()
        self.ys[insert] = ys                                      # :85
        self.insert += 1                                          # :86-87
        self.insert = self.insert % self.npairs
        return True

    def restart(self):                                            # lbfgs.py:89-95
        self.ys = [None] * self.npairs
        self.s = np.zeros((self.n, self.npairs), 'd')
        self.y = np.zeros((self.n, self.npairs), 'd')
        self.insert = 0

    def inverse(self, v):                                         # lbfgs.py:97-127
        dot = self.dot
        q = v.copy()
        s, y, ys, alpha = self.s, self.y, self.ys, self.alpha
        for i in range(self.npairs):
            k = (self.insert - 1 - i) % self.npairs
            if ys[k] is not None:
                alpha[k] = dot(s[:, k], q) / ys[k]                # :112
                q -= alpha[k] * y[:, k]                           # :113
        r = q
        if self.scaling:
            last = (self.insert - 1) % self.npairs
            if ys[last] is not None:
                self.gamma = ys[last] / dot(y[:, last], y[:, last])   # :119
                r *= self.gamma                                   # :120
        for i in range(self.npairs):
            k = (self.insert + i) % self.npairs
            if ys[k] is not None:
                beta = dot(y[:, k], r) / ys[k]                    # :125
                r += (alpha[k] - beta) * s[:, k]                  # :126
        return r

    def compact(self, v, use_gamma=True):                         # lbfgs.py:188-254
        """`use_gamma=False`: the same product with gamma = 1 whatever `scaling` says (what LBFGSOperator computes)."""
        dot = self.dot
        q = v.copy()
        r = v.copy()
        s, y, ys = self.s, self.y, self.ys
        prodn = 2 * self.npairs
        a = np.zeros(prodn)
        minimat = np.zeros([prodn, prodn])
        gamma = self.gamma if use_gamma else 1.0
        if self.scaling and use_gamma:
            last = (self.insert - 1) % self.npairs
            if ys[last] is not None:
                self.gamma = gamma = ys[last] / dot(y[:, last], y[:, last])    # :210
                r /= gamma                                        # :211
        paircount = 0
        for i in range(self.npairs):
            k = (self.insert + i) % self.npairs
            if ys[k] is not None:
                a[paircount] = dot(r[:], s[:, k])                 # :217
                paircount += 1
        j = 0
        for i in range(self.npairs):
            k = (self.insert + i) % self.npairs
            if ys[k] is not None:
                a[paircount + j] = dot(q[:], y[:, k])             # :224
                j += 1
        k_ind = 0
        for i in range(self.npairs):                              # :228-243
            k = (self.insert + i) % self.npairs
            if ys[k] is not None:
                minimat[paircount + k_ind, paircount + k_ind] = -ys[k]
                minimat[k_ind, k_ind] = dot(s[:, k], s[:, k]) / gamma
                l_ind = 0
                for j in range(i):
                    l = (self.insert + j) % self.npairs           # noqa: E741
                    if ys[l] is not None:
                        minimat[k_ind, paircount + l_ind] = dot(s[:, k], y[:, l])
                        minimat[paircount + l_ind, k_ind] = minimat[k_ind, paircount + l_ind]
                        minimat[k_ind, l_ind] = dot(s[:, k], s[:, l]) / gamma
                        minimat[l_ind, k_ind] = minimat[k_ind, l_ind]
                        l_ind += 1
                k_ind += 1
        if paircount > 0:
            rng = 2 * paircount
            b = np.linalg.solve(minimat[0:rng, 0:rng], a[0:rng])  # :247
        for i in range(paircount):
            k = (self.insert - paircount + i) % self.npairs
            r -= (b[i] / gamma) * s[:, k]                         # :251
            r -= b[i + paircount] * y[:, k]                       # :252
        return r
