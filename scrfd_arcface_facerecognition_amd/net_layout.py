"""The layer-table format in Python: a mirror of csrc/net.h (op types, op / tensor record words), csrc/conv.h (activations, epilogue flags) and
include/faceid.h (record sizes), with the headers' names, values and overlaps.  Constants only, plus the one statement of which words of an op
record name tensors.  tests/test_net_layout.py pins every name and value here to the headers, both ways."""

OP_WORDS, TENSOR_WORDS = 32, 8                     # FID_OP_WORDS, FID_TENSOR_WORDS

OP_STEM, OP_CONV, OP_MAXPOOL, OP_DWCONV, OP_STEMFUSED, OP_BBLOCK, OP_DWPW, OP_MBBLOCK, OP_STEMBLOCK, OP_LATFPN = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10

ACT_NONE, ACT_RELU, ACT_PRELU = 0, 1, 2
ACT = {"none": ACT_NONE, "relu": ACT_RELU, "prelu": ACT_PRELU}
CF_RES_UP2, CF_BORDER, CF_OUT_F32, CF_ARGMAX = 1, 2, 4, 8

# words of every op record
(W_TYPE, W_SRC, W_DST, W_RES, W_KH, W_KW, W_STRIDE, W_PAD, W_CIN, W_COUT, W_ACT, W_FLAGS, W_NSIG, W_WOFF, W_WBYTES, W_BOFF, W_SOFF, W_WROWS,
 W_GROUPS) = range(19)
W_F_MACS_LO, W_F_MACS_HI = 26, 27                  # every fused op: MACs per image of the group
# words 20.. mean what the op type says (csrc/net.h describes each)
W_F_W0, W_F_B0, W_F_W1, W_F_B1, W_F_W2, W_F_B2 = 20, 21, 22, 23, 24, 25                                    # OP_STEMFUSED
W_B_W1, W_B_B1, W_B_W2, W_B_B2, W_B_S1, W_B_ACT1 = 20, 21, 22, 23, 24, 25                                  # OP_BBLOCK
W_D_WOFF, W_D_BOFF, W_D_SOFF, W_D_ACT = 20, 21, 22, 23                                                     # OP_DWPW
W_M_W1, W_M_B1, W_M_S1, W_M_ACT1, W_M_DW, W_M_DWB, W_M_DWS, W_M_DWACT, W_M_GP = 20, 21, 22, 23, 24, 25, 28, 29, 30   # OP_MBBLOCK
W_S_W1, W_S_B1, W_S_S1, W_S_ACT0, W_S_DST2 = 20, 21, 22, 23, 24                                            # OP_STEMBLOCK
W_L_W0, W_L_B0, W_L_LAT = 20, 21, 22                                                                       # OP_LATFPN
W_X_DST2, W_X_ACT2, W_X_COUT1P = 20, 21, 22                                                                # OP_CONV + the shortcut as a second output
W_X_SRC2, W_X_T2, W_X_KW2, W_X_S2, W_X_W2OFF, W_X_B2OFF, W_X_SCOP = 23, 24, 25, 28, 29, 30, 31             # OP_CONV + the shortcut as extra K-steps

T_C, T_CP, T_H, T_W, T_DTYPE, T_SLOT, T_FLAGS = range(7)


def record_tensors(rec):
    """(tensor ids an op record reads, tensor ids it writes); the `+ 1` words hold id + 1, 0 = none"""
    kind = rec[W_TYPE]
    reads = [int(rec[w]) for w in (W_SRC, W_RES) if rec[w] >= 0]
    if kind == OP_CONV and rec[W_X_SRC2] > 0:
        reads.append(int(rec[W_X_SRC2]) - 1)
    writes = [int(rec[W_DST])]
    for op, w in ((OP_CONV, W_X_DST2), (OP_STEMBLOCK, W_S_DST2), (OP_LATFPN, W_L_LAT)):
        if kind == op and rec[w] > 0:
            writes.append(int(rec[w]) - 1)
    return reads, writes
