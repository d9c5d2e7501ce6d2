"""Shared pieces of the kernel-family GPU tests (test_gpu_conv_families.py, test_gpu_batch_shapes.py): the layer stacks, the table that
turns a test's family code into the autotuner hooks FID_FORCE_GEN / FID_FORCE_NS and into the check of WHICH family ran, and the activation-slot guard
(poison the rows at or beyond the batch of a net that runs below its max_batch, check them afterwards).  Plain module, no fixtures; the slot
arithmetic is pure Python on lower()'s tensor table, so tests/test_slot_guard_cpu.py checks it without a GPU."""
import numpy as np

from scrfd_arcface_facerecognition_amd.archs import Conv, Net
from scrfd_arcface_facerecognition_amd.lower import (OP_CONV, OP_LATFPN, OP_STEMBLOCK, T_CP, T_DTYPE, T_H, T_SLOT, T_W, W_DST, W_L_LAT, W_S_DST2, W_TYPE,
                                                     W_X_DST2, W_X_SRC2, W_X_W2OFF)


def _row(name, tup, env, **match):
    return {"name": name, "tuple": tup, "env": {"FID_" + k: str(v) for k, v in env.items()}, "match": match}


# The tests' own decode of a family code, once: the library's name of the variant and one plan tuple (gen bm bn bk ksplit ns) of it (tests/
# test_conv_variants_cpu.py checks both against the library), the autotuner hooks that force it, and the fields of a plans() row that say it ran.
# 59 = generation 5 with register-staged producers; 9x: conv3x3_wr and conv_ks; 9xx: conv3x3_wr on STRIP tiles.
FAMILIES = {
    0: _row("direct", (0, 0, 0, 0, 1, 0), {"FORCE_GEN": 0}, gen=0),
    1: _row("gemm.rs", (1, 128, 128, 64, 1, 4), {"FORCE_GEN": 1}, gen=1),
    2: _row("gemm.dma", (2, 128, 64, 64, 1, 4), {"FORCE_GEN": 2}, gen=2),
    3: _row("chunked", (3, 256, 64, 32, 1, 0), {"FORCE_GEN": 3}, gen=3),
    4: _row("pp", (4, 512, 48, 32, 1, 0), {"FORCE_GEN": 4}, gen=4),
    5: _row("pc", (5, 256, 96, 32, 1, 0), {"FORCE_GEN": 5}, gen=5),
    6: _row("gemm.pc", (6, 128, 64, 64, 1, 3), {"FORCE_GEN": 6}, gen=6),
    7: _row("pcr", (7, 256, 64, 32, 1, 0), {"FORCE_GEN": 7}, gen=7),
    8: _row("pc2", (8, 512, 64, 32, 1, 0), {"FORCE_GEN": 8}, gen=8),
    10: _row("s2", (10, 128, 96, 32, 1, 0), {"FORCE_GEN": 10}, gen=10),
    11: _row("gw", (11, 64, 256, 32, 1, 0), {"FORCE_GEN": 11}, gen=11),
    25: _row("gemm.dma.pf", (2, 64, 64, 64, 1, 5), {"FORCE_GEN": 2, "FORCE_NS": 5}, gen=2, ns=5),
    51: _row("pc.wahead", (5, 256, 64, 32, 1, 1), {"FORCE_GEN": 5, "FORCE_NS": 1}, gen=5, ns=1),
    59: _row("pc", (5, 256, 64, 32, 1, 0), {"FORCE_GEN": 5, "PC_RS": 1}, gen=5),
    91: _row("wr.one", (9, 256, 64, 32, 1, 0), {"FORCE_GEN": 9, "FORCE_NS": 1}, gen=9, ns=0, bm=256),
    92: _row("wr.pair", (9, 512, 128, 32, 1, 0), {"FORCE_GEN": 9, "FORCE_NS": 2}, gen=9, ns=0, bm=512),
    93: _row("wr.resident", (9, 256, 128, 32, 1, 1), {"FORCE_GEN": 9, "FORCE_NS": 3}, gen=9, ns=1),
    94: _row("wr.ring4", (9, 256, 64, 32, 1, 4), {"FORCE_GEN": 9, "FORCE_NS": 4}, gen=9, ns=4),
    96: _row("ks", (9, 256, 64, 32, 1, 6), {"FORCE_GEN": 9, "FORCE_NS": 6}, gen=9, ns=6, bm=256),
    97: _row("ks.2perwg", (9, 512, 64, 32, 1, 6), {"FORCE_GEN": 9, "FORCE_NS": 7}, gen=9, ns=6, bm=512),
    98: _row("ks.strip", (9, 256, 64, 32, 1, 7), {"FORCE_GEN": 9, "FORCE_NS": 8}, gen=9, ns=7),
    909: _row("wr.strip.one", (9, 256, 64, 32, 1, 8), {"FORCE_GEN": 9, "FORCE_NS": 9}, gen=9, ns=8, bm=256, bn=64),
    929: _row("wr.strip.pair", (9, 512, 128, 32, 1, 8), {"FORCE_GEN": 9, "FORCE_NS": 29}, gen=9, ns=8, bm=512, bn=128),
    939: _row("wr.strip.one128", (9, 256, 128, 32, 1, 8), {"FORCE_GEN": 9, "FORCE_NS": 39}, gen=9, ns=8, bm=256, bn=128),
    910: _row("wr.strip.resident", (9, 256, 256, 32, 1, 9), {"FORCE_GEN": 9, "FORCE_NS": 10}, gen=9, ns=9),
}


def force_family(monkeypatch, code):
    """a test's family code -> the autotuner hooks of its FAMILIES row (and none of another row's)"""
    for k in ("FID_FORCE_GEN", "FID_FORCE_NS", "FID_PC_RS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FAMILIES[code]["env"].items():
        monkeypatch.setenv(k, v)


def forced_ran(cn, code, batch=None):
    """ops of the net whose pick is the kernel variant the test forced (code: a FAMILIES row).  The hooks only restrict the candidates where the variant applies; a test
    that asserted nothing about the pick would pass on another family's result.  batch: only the picks made for that batch size (a net that ran several)."""
    match = FAMILIES[code]["match"]
    return [p["name"] for p in cn.plans() if all(p[k] == v for k, v in match.items()) and (batch is None or p["batch"] == batch)]


def stack(hw, chans, res=True):
    net = Net("t", hw, 127.5, 1.0 / 128.0)
    net.add(Conv("s", "input", 3, 64, act="relu"))
    src, cin = "s", 64
    for i, c in enumerate(chans):
        net.add(Conv(f"a{i}", src, cin, c, act="prelu", pre_bn=(i == 1)))
        net.add(Conv(f"b{i}", f"a{i}", c, c, act="relu", res=f"a{i}" if res else None))
        src, cin = f"b{i}", c
    net.outputs = [src]
    return net


# ---- activation slots: rows at or beyond the batch ------------------------------------------------------------------------------------

# both as fp16 and as fp32 pairs: 0x7BFF = 65504 / a large finite value, 0x7E00 = NaN / NaN
POISON = {"max": 0x7BFF, "nan": 0x7E00}


def slot_table(low):
    """(slot of every tensor, bytes per image of every tensor, bytes per image of every slot) from lower()'s tensor table.  T_SLOT is the
    slot (a view's record already names its base's slot), a tensor's image is H x W x Cp elements of 2 (fp16) or 4 (fp32, dtype 1) bytes,
    every tensor of a slot starts at the slot's base, and a slot's image is the largest of its tensors' (csrc/net.hip, fid_net_create)."""
    t_slot, t_bytes, s_bytes = [], [], {}
    for Cp, H, W, dtype, slot in (tuple(int(r[w]) for w in (T_CP, T_H, T_W, T_DTYPE, T_SLOT)) for r in low.tensors):
        b = H * W * Cp * (4 if dtype == 1 else 2)
        t_slot.append(slot)
        t_bytes.append(b)
        s_bytes[slot] = max(s_bytes.get(slot, 0), b)
    return t_slot, t_bytes, s_bytes


def guard_regions(low, b, max_batch):
    """{slot: (first guard byte, end)}: the bytes of a slot no image below b of ANY of its tensors occupies, up to the allocation's end"""
    _, _, s_bytes = slot_table(low)
    return {s: (b * n, max_batch * n) for s, n in s_bytes.items()}


def own_data_tensors(low):
    """names of the tensors that still hold their own rows after a run: the last tensor written into its slot (earlier tenants were
    overwritten), except where that writer is a block-shortcut conv the consuming conv may absorb (then it does not run at all)"""
    names = {i: n for n, i in low.tensor_id.items()}
    last = {}
    for r in low.ops:
        kind = int(r[W_TYPE])
        dsts = [int(r[W_DST])]
        for op, word in ((OP_CONV, W_X_DST2), (OP_STEMBLOCK, W_S_DST2), (OP_LATFPN, W_L_LAT)):     # second outputs: tensor id + 1
            if kind == op and r[word] > 0:
                dsts.append(int(r[word]) - 1)
        maybe_skipped = kind == OP_CONV and r[W_X_SRC2] == 0 and r[W_X_W2OFF] > 0                 # this word of a shortcut op: its consumer + 1
        for d in dsts:
            last[int(low.tensors[d][T_SLOT])] = None if maybe_skipped else d
    return sorted(names[d] for d in last.values() if d is not None)


class SlotGuard:
    """The rows at or beyond batch b of every activation slot of a CompiledNet built for more: poison() fills them with a 16-bit pattern,
    check() asserts that a run left every byte of them alone.  A kernel only receives the tensor pointer and the batch: a store into row b
    is a heap overrun on a net whose max_batch is b."""

    def __init__(self, ctx, cn, b, pattern):
        assert 0 < b < cn.max_batch
        self.ctx, self.cn, self.b, self.word = ctx, cn, b, np.uint16(POISON[pattern])
        t_slot, _, _ = slot_table(cn.low)
        by_id = {i: n for n, i in cn.low.tensor_id.items()}
        self.regions = []
        for slot, (lo, hi) in sorted(guard_regions(cn.low, b, cn.max_batch).items()):
            ptr, _, _ = cn.tensor(by_id[t_slot.index(slot)])          # any tensor of the slot: all start at its base
            assert lo % 2 == 0 and hi > lo
            self.regions.append((slot, lo, ctx.borrow(ptr + lo, ((hi - lo) // 2,), np.uint16)))

    def poison(self):
        for _, _, buf in self.regions:
            buf.upload(np.full(buf.shape, self.word, np.uint16))
        return self

    def check(self, what=""):
        for slot, lo, buf in self.regions:
            got = buf.download()
            bad = np.flatnonzero(got != self.word)
            if bad.size:
                byte = lo + 2 * int(bad[0])
                per = lo // self.b
                raise AssertionError(f"{what}: slot {slot} written beyond batch {self.b}: first changed byte {byte} (image row {byte // per}, "
                                     f"offset {byte % per} of {per}), {bad.size} of {got.size} guard words changed, "
                                     f"0x{int(got[bad[0]]):04x} instead of 0x{int(self.word):04x}")
