#!/usr/bin/env python3
"""development: the tile plans of the dense 3x3 forward / input-gradient kernels over a grid of shapes, one key line per query followed by
the plan line(s) the library prints for it (conv_mfma_body.h conv_plan_note: candidate, staging width, RT, bpi, nseg, Q, single, parts,
grid, LDS bytes).  Needs a DEV=1 library and no GPU: every call is a query.  Compare two libraries by running it once each (EAS_LIB) and
diffing the files:

  EAS_CONV_PLAN=1 python scripts/dev_conv3_plans.py 2> plans.txt"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eas_snn_amd import _lib  # noqa: E402

NIS = (1, 2, 3, 5, 64, 160, 192)
CH = (8, 16, 24, 32, 40, 48, 64, 72, 96, 128, 192, 256, 384, 512)
MAPS = ((6, 4), (8, 10), (10, 12), (12, 16), (16, 20), (32, 40), (64, 80), (128, 160), (8, 96), (8, 240), (8, 320), (12, 320), (4, 640), (192, 320))


def key(s):
    os.write(2, (s + '\n').encode())


def main():
    L = _lib.lib()
    for NI in NIS:
        for Cin in CH:
            for Cout in CH:
                for H, W in MAPS:
                    for s in (1, 2):
                        for xt in (1, 2, 3):
                            key(f'fwd {NI} {Cin} {Cout} {H} {W} s{s} xt{xt} -> {L.eas_conv_fwd_supported(NI, Cin, Cout, H, W, 3, s, xt)}')
                        # the fused eval step: spike planes over T = 3 / 5 steps (time-major), one shared fp32 frame set in one / three terms
                        for T, xt, sh in ((3, 2, 0), (5, 2, 0), (3, 1, 1), (3, 3, 1)):
                            key(f'lif {T} {NI} {Cin} {Cout} {H} {W} s{s} xt{xt} sh{sh} -> '
                                f'{L.eas_conv_bn_lif_eval_supported(T, NI, Cin, Cout, H, W, 3, s, xt, sh)}')
                    key(f's2d {NI} {Cin} {Cout} {H} {W} -> {L.eas_conv_dgrad_s2_supported(NI, Cin, Cout, H, W)}')
    # the three pyramid levels of the 256x320, 384x640 and 192x256 canvases as one group
    for canvas in ((256, 320), (384, 640), (192, 256)):
        for NI in (2, 32, 64, 96, 160, 192, 224):
            for Cin, Cout in ((64, 64), (96, 96), (128, 128), (192, 192), (256, 256), (128, 256), (256, 128), (64, 128), (192, 96), (320, 320)):
                pr = (_lib.EasConvProblem * 3)()
                for p, d in enumerate((8, 16, 32)):
                    pr[p].NI, pr[p].Cin, pr[p].Cout, pr[p].Hi, pr[p].Wi = NI, Cin, Cout, canvas[0] // d, canvas[1] // d
                nb = (C.c_int * 3)()
                rc = L.eas_conv_fwd_group_plan(pr, 3, 3, 3, nb)
                key(f'group {canvas[0]}x{canvas[1]} {NI} {Cin} {Cout} -> {rc} nb {list(nb)}')


if __name__ == '__main__':
    main()
