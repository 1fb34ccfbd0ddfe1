"""CPU model of FV_OPT_FLAT_GENERATIONS (flash_viterbi_amd/csrc/fv_full.hip, run_flat_full): speculate every right-hand
pass from the whole-sequence chain, resolve generation by generation, fall back from the first generation that cannot
be committed.  Built on the oracle's single-pass primitive (full_forward); shared by the CPU and the GPU tests."""
import numpy as np

from flash_viterbi_amd import decoder


class PassRunner:
    """full_forward + back-track of one pass, remembered by (L, R, start state, end state)."""

    def __init__(self, m, ob):
        self.m, self.ob, self.fwd = m, ob, {}

    def forward(self, L, R, init):
        key = (L, R, init)
        if key not in self.fwd:
            self.fwd[key] = self.m.full_forward(self.ob, L, R, init)
        return self.fwd[key]

    def chain(self, L, R, init, end):
        """c[L..R-1] of the pass [L, R] started from `init` at time L-1 and back-tracked from `end` at time R."""
        _, args = self.forward(L, R, init)
        out, st = [], int(end)
        for j in range(R, L, -1):
            st = int(args[j - L - 1][st]) if st >= 0 else -1
            out.append(st)
        return out[::-1]


def flat_decode_cpu(m, ob, n_split, K, poison=None):
    """Returns (answers, flat passes, missed passes of the first generation with a miss, that generation or -1)."""
    T = len(ob)
    plan = decoder.plan_passes(T, n_split)
    run = PassRunner(m, ob)
    ans = np.zeros(T, dtype=np.int64)
    row, _ = run.forward(0, T - 1, -1)
    ans[T - 1] = int(np.argmax(row))
    ans[:T - 1] = run.chain(0, T - 1, -1, ans[T - 1])
    S = ans.copy()
    if poison is not None and poison >= 0:
        S[poison] = (S[poison] + 1) % K
    right = [p for p in plan if p[2] >= 1]
    chains = {(L, R): run.chain(L, R, int(S[L - 1]), int(S[R])) for (L, R, _, _) in right}
    first_miss, missed = -1, 0
    gens = sorted({p[2] for p in right})
    for g in gens:
        mine = [p for p in right if p[2] == g]
        bad = [p for p in mine if S[p[0] - 1] != ans[p[0] - 1] or S[p[1]] != ans[p[1]]]
        if bad:
            first_miss, missed = g, len(bad)
            break
        for (L, R, _, _) in mine:
            ans[L:R] = chains[(L, R)]
    if first_miss >= 0:
        for g in [x for x in gens if x >= first_miss]:
            for (L, R, _, _) in [p for p in right if p[2] == g]:
                ans[L:R] = run.chain(L, R, int(ans[L - 1]), int(ans[R]))
    return ans, len(right), missed, first_miss
