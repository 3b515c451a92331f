"""The products of ff/montx_dev.hpp (operator*, mul2, mul_add, sqr2, sqr -- the column blocks of ff/montx_blocks.hpp),
column by column on Python integers, and the operands that sit at the edges of each form's contract.  Shared by the host
test of the blocks' plain-C bodies (tests/test_montx_blocks.py) and the device test of their asm statements
(tests/test_g2_device_gpu.py): both feed the same operands and require the same limbs."""
import numpy as np

# (NL, LB) of the field `which` of a curve: 0 = the G1 bucket field, 1 = the base field of the G2 bucket field
LIMBS = {("BLS12_381", 0): (14, 28), ("BLS12_377", 0): (14, 28), ("BN254", 0): (9, 29), ("BN254", 1): (10, 28),
         ("PALLAS", 0): (9, 29), ("VESTA", 0): (9, 29), ("BLS12_381", 1): (14, 28), ("BLS12_377", 1): (14, 28)}


class Model:
    """montx_dev's products, column by column, on Python integers"""
    def __init__(self, NL, LB, fat_m_ok, plimbs):
        self.NL, self.LB, self.fat_m_ok, self.pl = NL, LB, fat_m_ok, plimbs
        self.MASK = (1 << LB) - 1
        self.p = sum(v << (LB * j) for j, v in enumerate(plimbs))
        self.M0 = (-pow(self.p, -1, 1 << 32)) % (1 << 32)           # -1/p mod 2^32; its low LB bits: -1/p mod 2^LB
        self.PINV = self.M0 & self.MASK

    def digit(self, A, k, fat):
        if fat and self.fat_m_ok and k < self.NL - 1:
            return ((A & 0xffffffff) * self.M0) & 0xffffffff
        return ((A & 0xffffffff) * self.PINV) & 0xffffffff & self.MASK

    def reduce(self, column, fat=False):
        """column(k) = the sum of the operands' partial products of column k"""
        NL, pl = self.NL, self.pl
        m, r, A = [], [], 0
        for k in range(2 * NL):
            if k <= 2 * NL - 2:
                A += column(k)
                A += sum(m[i] * pl[k - i] for i in range(max(0, k - NL + 1), min(k, NL)))
            assert A < 1 << 64, "a column left the 64-bit accumulator"
            if k < NL:
                m.append(self.digit(A, k, fat))
                A += m[k] * pl[0]
                assert A < 1 << 64
            else:
                r.append(A & self.MASK)
            A >>= self.LB
        return r

    def mul(self, a, b, fat=False):
        NL = self.NL
        return self.reduce(lambda k: sum(a[i] * b[k - i] for i in range(max(0, k - NL + 1), min(k, NL - 1) + 1)), fat)

    def mul_add(self, a0, b0, a1, b1):
        NL = self.NL
        return self.reduce(lambda k: sum(a0[i] * b0[k - i] + a1[i] * b1[k - i] for i in range(max(0, k - NL + 1), min(k, NL - 1) + 1)))

    def sqr(self, a, fat=False):
        NL = self.NL
        d = [(x << 1) & 0xffffffff for x in a]

        def column(k):
            s = 0
            for i in range(max(0, k - NL + 1), min(k, NL - 1) + 1):
                j = k - i
                if i < j:
                    s += a[i] * d[j]
                elif i == j:
                    s += a[i] * a[i]
            return s
        return self.reduce(column, fat)

    def limbs(self, v):
        return [(v >> (self.LB * j)) & self.MASK if j < self.NL - 1 else v >> (self.LB * j) for j in range(self.NL)]

    def val(self, l):
        return sum(int(x) << (self.LB * j) for j, x in enumerate(l))


def check_forms(run, info, tag, rng, n=160):
    """All seven forms at the edges of their contracts, then on random operands, limb for limb against the model.
    info: the 64 integers of emu_blocks_info / sppark_devtest_blocks_info (NL, LB, FAT_M_OK, MA_A0, MA_A1, SQR_L, ..., the
    modulus' limbs from index 8); run(form, A0, B0, A1, B1) -> (r0, r1): (n, NL) uint32 arrays in and out."""
    NL, LB, fat_ok, MA0, MA1, SQRL = (int(v) for v in info[:6])
    M = Model(NL, LB, bool(fat_ok), [int(v) for v in info[8:8 + NL]])
    p, MASK = M.p, M.MASK
    R = 1 << (LB * NL)
    Rinv = pow(R, -1, p)
    # Limb patterns at the edge of a contract: every limb BUT THE TOP at its bound; the top limb is the modulus' own, so that the
    # value stays below 2p + (the products' contracts bound the value as well: the result must fit NL normalised limbs)
    ptop = M.pl[NL - 1]
    const = lambda v: [v] * (NL - 1) + [ptop]
    norm_edges = [[0] * NL, M.limbs(1), M.limbs(p - 1), M.limbs(p), M.limbs(2 * p - 1), const(MASK), M.limbs(p - 1)[:1] + const(MASK)[1:]]

    def norm(i):
        return norm_edges[i] if i < len(norm_edges) else M.limbs(rng.randrange(2 * p))

    def fat(i, top):                                            # limbs <= top
        edges = [const(top), [0] * NL, [top if j % 2 else 0 for j in range(NL - 1)] + [ptop], [0 if j % 2 else top for j in range(NL - 1)] + [0],
                 M.limbs(p - 1)]
        return edges[i] if i < len(edges) else [rng.randrange(top + 1) for _ in range(NL - 1)] + [rng.randrange(ptop + 1)]
    ne = len(norm_edges)
    FATL = (1 << 31) - 1
    # (form, left-operand limb bounds, quotient digits unmasked, model)
    cases = [(0, FATL, FATL, (False, False)), (1, FATL, FATL, (False, False)), (2, MASK, MASK, (True, True)), (3, MASK, FATL, (True, False)),
             (4, (MA0 << LB) - 1, (MA1 << LB) - 1, None), (5, MASK, MASK, (True, True)), (6, (SQRL << LB) - 1, MASK, (False, False))]
    for form, top0, top1, fatm in cases:
        left_norm0, left_norm1 = top0 == MASK, top1 == MASK
        # every edge of the left operands against every edge of the right ones, then random
        a0 = [norm(i % ne) if left_norm0 else fat(i % 5, top0) for i in range(n)]
        a1 = [norm((i + 3) % ne) if left_norm1 else fat((i + 1) % 5, top1) for i in range(n)]
        b0 = [norm((i // 5) % ne) for i in range(n)]
        b1 = [norm((i // 5 + 2) % ne) for i in range(n)]
        for i in range(ne * 5, n):
            a0[i] = norm(99) if left_norm0 else fat(99, top0); a1[i] = norm(99) if left_norm1 else fat(99, top1)
            b0[i] = norm(99); b1[i] = norm(99)
        arr = lambda x: np.array(x, dtype=np.uint32)
        r0, r1 = run(form, arr(a0), arr(b0), arr(a1), arr(b1))
        for i in range(n):
            if form == 4:
                e0, e1 = M.mul_add(a0[i], b0[i], a1[i], b1[i]), None
                v0 = M.val(a0[i]) * M.val(b0[i]) + M.val(a1[i]) * M.val(b1[i])
            elif form == 5:
                e0, e1 = M.sqr(a0[i], True), M.sqr(a1[i], True)
                v0, v1 = M.val(a0[i]) ** 2, M.val(a1[i]) ** 2
            elif form == 6:
                e0, e1 = M.sqr(a0[i]), None
                v0 = M.val(a0[i]) ** 2
            else:
                e0 = M.mul(a0[i], b0[i], fatm[0])
                e1 = M.mul(a1[i], b1[i], fatm[1]) if form else None
                v0, v1 = M.val(a0[i]) * M.val(b0[i]), M.val(a1[i]) * M.val(b1[i])
            assert [int(x) for x in r0[i]] == e0, (tag, form, i)
            assert M.val(e0) % p == v0 * Rinv % p and max(e0) <= MASK
            if e1 is not None:
                assert [int(x) for x in r1[i]] == e1, (tag, form, i, "second product")
                assert M.val(e1) % p == v1 * Rinv % p and max(e1) <= MASK
