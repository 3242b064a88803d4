"""LDS bank check of the dynamic int8 conv's A-operand reads (csrc/conv_dyn.hip,
DESIGN §24), in the model of tools/lds_banks.py (host only).

Lane (p = l % 16, g = l / 16) of v_mfma_i32_16x16x64_i8 reads 16 bytes of
pixel p at K unit 4 s + g of step s; pixel p = 4 q + e is row e >> 1, column
2 q + (e & 1) of the 2 x 8 tile; unit u is tap u / ncg, channel group u % ncg.
Prints the cycles of the worst ds_read_b128 (4 = conflict-free) for every
count of 16-channel groups of a chunk and every block width.

    python tools/lds_banks_dyn.py
"""
from lds_banks import read_cycles


def pixel_stride(ncg):   # cd_pixel_stride
    return 16 * (ncg + (ncg == 1) if ncg % 4 else (ncg if ncg % 8 else ncg + 2))


def row_stride(ncg, lcols):   # cd_row_stride
    return lcols * pixel_stride(ncg) + ((16 if ncg == 1 else 96) if ncg % 4 else (32 if ncg % 8 else 64))


def worst(ncg, lcols):
    ps, rs, nu, w = pixel_stride(ncg), row_stride(ncg, lcols), 9 * ncg, 0
    for s in range((nu + 3) // 4):
        addrs = []
        for l in range(64):
            p, g = l & 15, l >> 4
            u = 4 * s + g if 4 * s + g < nu else 0
            tap, cg = u // ncg, u % ncg
            addrs.append(((p >> 1 & 1) + tap // 3) * rs + (2 * (p >> 2) + (p & 1) + tap % 3) * ps + 16 * cg)
        w = max(w, read_cycles(addrs))
    return w


def handoff_ways(ncg, lcols):
    """Worst N-way conflict of the pair kernel's hand-off ds_write_b32 into the
    mid band (csrc/conv_dyn_pair.hip; width 32: csrc/conv_dyn_pair32.hip,
    DESIGN §26, whose x band and mid band are both this layout), in the write model of
    lds_banks.conv1_write_ways (2 groups of 32 lanes, bank (a / 4) mod 32): lane
    (c16, g) writes channels 4 (c16 / 4) .. + 3 of position c16 % 4 of window g."""
    ps, rs, worst_ways = pixel_stride(ncg), row_stride(ncg, lcols), 0
    for half in range(2):
        banks = {}
        for l in range(32 * half, 32 * half + 32):
            e, q, g = l & 3, (l & 15) >> 2, l >> 4
            a = (e >> 1) * rs + (2 * g + (e & 1)) * ps + 4 * q
            banks.setdefault((a // 4) % 32, set()).add(a // 4)
        worst_ways = max(worst_ways, max(len(v) for v in banks.values()))
    return worst_ways


if __name__ == "__main__":
    for ncg in range(1, 17):
        print(f"ncg {ncg:2d} (cin chunk {16 * ncg:3d}): PS {pixel_stride(ncg):3d} B, worst cycles at block widths "
              f"8 / 16 / 32: {' / '.join(str(worst(ncg, 8 * wpx + 2)) for wpx in (1, 2, 4))}; "
              f"pair hand-off writes at widths 8 / 16 / 32: "
              f"{' / '.join(str(handoff_ways(ncg, 8 * pgx + 2)) for pgx in (1, 2, 4))}-way")
