"""LDS bank-conflict check of the conv patch reads (diagnostic, host only).

For a ConvCfg patch layout (PSP / RPAD / SPAD / SPLIT, csrc/conv3x3.hip) and
an MFMA operand shape, computes every lane's ds_read_b128 address of every
B fragment (tap, cin block, pixel block) and the LDS cycles per
wave-instruction from MI355X_MICROARCH.md §LDS: a ds_read_b128 is served in
four lane groups of 16, one cycle per group when the group's 64 dwords fall
on distinct banks ((a / 4) mod 64), N cycles when a bank sees N distinct
dwords.

    python tools/lds_banks.py            # the headline layouts, both shapes
    python tools/lds_banks.py --search   # search PSP / RPAD / SPAD for 16x16x64

Shapes: '32' = v_mfma_i32_32x32x32_i8 (lane l: pixel l % 32, K bytes
16 (l / 32) + 32 kk), '16' = v_mfma_i32_16x16x64_i8 (lane l: pixel l % 16,
K bytes 16 (l / 16)).
"""
from __future__ import annotations

import argparse
import itertools

G0 = [0, 1, 2, 3, 12, 13, 14, 15] + list(range(20, 28))
G1 = list(range(4, 12)) + [16, 17, 18, 19] + list(range(28, 32))
GROUPS = [G0, G1, [l + 32 for l in G0], [l + 32 for l in G1]]


class Cfg:
    def __init__(self, cin, hw, pool, wpx, psp, rpad, spad, split, segs=1, name=""):
        self.cin, self.W, self.H, self.pool, self.wpx = cin, hw, hw, pool, wpx
        self.psp, self.rpad, self.spad, self.split, self.segs = psp, rpad, spad, split, segs
        self.name = name
        self.PS = cin + psp
        self.PCOLS = hw + 2
        self.PROWS = hw + 2
        self.HALF = (self.PCOLS + 1) // 2
        self.RS = self.PCOLS * self.PS + rpad
        self.SS = self.PROWS * self.RS + spad
        self.patch = segs * self.SS

    def slot(self, seg, prow, pcol):
        cpos = ((pcol & 1) * self.HALF + (pcol >> 1)) if self.split else pcol
        return seg * self.SS + prow * self.RS + cpos * self.PS

    def delta(self, tap, jpar):
        r, s = tap // 3, tap % 3
        dc = s
        if self.split:
            dc = 0 if s == 0 else (1 if s == 2 else ((1 - self.HALF) if jpar else self.HALF))
        return r * self.RS + dc * self.PS

    # pixel of (wave wp, block j, lane pixel p) -> (seg, prow, pcol, column parity)
    def pixel(self, shape, wp, j, p):
        if shape == "32":
            if self.pool:
                PW, PR = self.W // 2, self.H // 2
                q = wp * 32 + p
                seg = q // (PR * PW)
                return seg, 2 * ((q // PW) % PR) + (j >> 1), 2 * (q % PW) + (j & 1), j & 1
            m = (wp * 4 + j) * 32 + p
            return m // (self.H * self.W), (m // self.W) % self.H, m % self.W, 0
        if self.pool:
            PW, PR = self.W // 2, self.H // 2
            q = wp * 32 + (j >> 2) * 16 + p
            jq = j & 3
            seg = q // (PR * PW)
            return seg, 2 * ((q // PW) % PR) + (jq >> 1), 2 * (q % PW) + (jq & 1), jq & 1
        m = (wp * 8 + j) * 16 + p
        return m // (self.H * self.W), (m // self.W) % self.H, m % self.W, 0


def read_cycles(addrs):
    """LDS cycles of one ds_read_b128 wave-instruction (64 byte addresses)."""
    cyc = 0
    for g in GROUPS:
        banks = {}
        for l in g:
            d0 = addrs[l] // 4
            for t in range(4):
                banks.setdefault((d0 + t) % 64, set()).add(d0 + t)
        cyc += max(len(v) for v in banks.values())
    return cyc


def check(cfg, shape):
    """(worst, mean) cycles over every B-fragment read of the layer."""
    nj = 4 if shape == "32" else 8
    kks = (0, 1) if shape == "32" else (0,)
    worst, tot, n = 0, 0, 0
    for wp in range(cfg.wpx):
        for j in range(nj):
            for tap in range(9):
                for cb in range(cfg.cin // 64):
                    for kk in kks:
                        addrs = []
                        for l in range(64):
                            if shape == "32":
                                p, k = l & 31, (l >> 5) * 16 + kk * 32
                            else:
                                p, k = l & 15, (l >> 4) * 16
                            seg, pr, pc, par = cfg.pixel(shape, wp, j, p)
                            addrs.append(cfg.slot(seg, pr + (0 if cfg.pool else 1) * 0, pc) +
                                         cfg.delta(tap, par) + cb * 64 + k)
                        c = read_cycles(addrs)
                        worst = max(worst, c)
                        tot += c
                        n += 1
    return worst, tot / n


# the headline's patch layouts (ConvCfg arguments in conv3x3.hip)
HEADLINE = [
    ("conv2 (Conv2Cfg)", dict(cin=64, hw=32, pool=True, wpx=4, psp=32, rpad=0, spad=0, split=True, segs=1)),
    ("conv2 (r04 patch)", dict(cin=64, hw=32, pool=True, wpx=4, psp=16, rpad=96, spad=0, split=True, segs=1)),
    ("conv3 (WsA3)", dict(cin=64, hw=16, pool=False, wpx=2, psp=16, rpad=96, spad=0, split=False)),
    ("conv4 (WsB4)", dict(cin=128, hw=16, pool=True, wpx=2, psp=16, rpad=32, spad=0, split=True)),
    ("conv5 (WsA5)", dict(cin=128, hw=8, pool=False, wpx=1, psp=16, rpad=224, spad=0, split=False, segs=2)),
    ("conv6 (WsB6)", dict(cin=256, hw=8, pool=True, wpx=1, psp=16, rpad=32, spad=64, split=True, segs=2)),
]


def conv2_tile(kw):
    # conv12's conv2 runs half-image tiles: 16 output rows of 32 (R = 16)
    c = Cfg(**kw)
    c.H = 16
    c.PROWS = 18
    c.SS = c.PROWS * c.RS + c.spad
    return c


def make(name, kw):
    return conv2_tile(kw) if name.startswith("conv2") else Cfg(**kw, name=name)


# conv2's resident weights (conv12, conv_mainloop_res16): chunk s at s * 4096,
# row r (cout) 64 B, its 16-B slot c stored at slot c ^ swz(r)
def res16_swz(r):
    return (4 - ((r >> 2) & 3)) & 3


def ring_swz(r):
    return (r >> 2) & 3


def check_a16(swz=res16_swz):
    """(worst, mean) cycles over the A-fragment reads of conv2's 16x16x64 loop:
    lane (p, g) reads row 16 i + p, K bytes 16 g .. 16 g + 15, of every chunk."""
    worst, tot, n = 0, 0, 0
    for s in range(9):
        for i in range(4):
            addrs = []
            for l in range(64):
                p, g = l & 15, l >> 4
                r = 16 * i + p
                addrs.append(s * 4096 + r * 64 + ((g ^ swz(r)) << 4))
            c = read_cycles(addrs)
            worst, tot, n = max(worst, c), tot + c, n + 1
    return worst, tot / n


def conflicted(name, kw, shape="16"):
    """Number of conflicted B-fragment reads (more than 4 cycles) of a layout."""
    c = make(name, kw)
    nj = 4 if shape == "32" else 8
    bad = 0
    for wp in range(c.wpx):
        for j in range(nj):
            for tap in range(9):
                addrs = []
                for l in range(64):
                    p, k = (l & 15, (l >> 4) * 16) if shape == "16" else (l & 31, (l >> 5) * 16)
                    seg, pr, pc, par = c.pixel(shape, wp, j, p)
                    addrs.append(c.slot(seg, pr, pc) + c.delta(tap, par) + k)
                bad += read_cycles(addrs) > 4
    return bad


def conv1_write_ways(cfg):
    """Worst N-way conflict of the conv12 producer's ds_write_b32 into conv2's
    patch: 2 groups of 32 lanes, bank (a / 4) mod 32; lane (l32, hi) writes
    dword hi of a channel group of pixel column l32 + 1 of one patch row."""
    worst = 0
    for hi in range(2):
        banks = {}
        for l32 in range(32):
            a = cfg.slot(0, 1, l32 + 1) + 4 * hi
            banks.setdefault((a // 4) % 32, set()).add(a // 4)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def conv12_lds(cfg):
    """Conv12P's LDS plan (bytes): the two half-image patches around their one
    shared padding row, the resident weights, two input windows, the tables."""
    rows = 2 * cfg.PROWS - 1
    patches = rows * cfg.RS
    wres, win, tab = 9 * 64 * 64, 2 * 20 * 40 * 4, 2 * 768 + 256 + 2048 + 256
    total = patches + wres + win + tab
    return dict(rows=rows, row_stride=cfg.RS, patches=patches, weights=wres, windows=win, tables=tab,
                total=total, total_u8=total + 768, limit=160 * 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    args = ap.parse_args()
    for name, kw in HEADLINE:
        c = make(name, kw)
        for shape in ("32", "16"):
            w, m = check(c, shape)
            print(f"{name:18s} {shape}x{shape}: worst {w} cyc (4 = conflict-free), mean {m:.2f}, "
                  f"patch {c.patch} B")
    # conv12's conv2 on the 16x16x64 MFMA: B and A fragments, conv1's writes, the LDS plan
    name, kw = HEADLINE[0]
    c2 = make(name, kw)
    print(f"conv2 16x16 B fragments: {conflicted(name, kw)} conflicted reads of {c2.wpx * 8 * 9}")
    for label, swz in (("res16_swz", res16_swz), ("ring swizzle", ring_swz)):
        w, m = check_a16(swz)
        print(f"conv2 16x16 A fragments ({label}): worst {w} cyc, mean {m:.2f}")
    for nm, k2 in HEADLINE[:2]:
        print(f"{nm}: conv1's ds_write_b32 into the patch {conv1_write_ways(make(nm, k2))}-way "
              "(2-way is free, 4-way 2x, 8-way 4x the LDS cycles)")
    plan = conv12_lds(c2)
    print("conv12 LDS plan:", ", ".join(f"{k} {v}" for k, v in plan.items()))
    if not args.search:
        return
    for name, kw in HEADLINE:
        best = []
        for psp, rpad, spad in itertools.product((16, 32, 48, 80), range(0, 257, 16), (0, 16, 32, 64, 96)):
            if kw["segs"] == 1 and spad:
                continue
            k2 = dict(kw, psp=psp, rpad=rpad, spad=spad)
            c = make(name, k2)
            w, m = check(c, "16")
            best.append((m, w, c.patch, psp, rpad, spad))
        best.sort(key=lambda t: (t[0], t[2]))
        print(name, "best 16x16 layouts (mean cyc, worst, patch B, PSP, RPAD, SPAD):", best[:5])


if __name__ == "__main__":
    main()
