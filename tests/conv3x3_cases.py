"""The 3x3 convolution kernels' instance table: which shape reaches which compiled instance, in which run-time form.

Shared by tests/test_cpu_conv3x3_plan.py (no GPU: every row lands where it promises, by the launch's own planner through eas_conv_fwd_plan /
eas_conv_dgrad_s2_plan / eas_conv_fwd_group_tile_plan; a walk over a search box finds no instance or run-time form without a row) and
tests/test_gpu_conv3x3_instances.py (every row is launched and compared with fp64).  One table, checked from both sides.

An instance is a kernel family, its template arguments and the run-time form of the launch:
  forward       conv_fwd_mfma_kernel<9, S, XT, 1, WN, WVM, WVN, 16, VEC, NIT, PL, 0>; key (S, terms, VEC, candidate, single, parts, nseg > 1,
                ragged): terms 3 = fp32 in three bf16 terms, 1 = one term -- fp32 small integers (x_terms 1) AND spike planes (x_terms 2,
                PL), two compiled instances that the planner treats alike; candidate = index in TILES (dispatch_tile's table); single = the
                single-buffered patch; parts = column parts; nseg > 1 = a tile of several whole images; ragged = a last tile short of rows
  stride-2 input gradient   conv_dgrad_s2c_kernel<WN, WVM, WVN, VEC>; key (candidate in S2D_TILES, VEC, bpi > 1, nseg > 1, short): bpi > 1 =
                an image cut into several tiles, short = the last of them short of rows
  grouped       conv3x3_group_kernel<3, WN, WVM, WVN, 2, 0, ConvGeomCore>; key = candidate in GROUP_TILES
"""
import ctypes as C

TILES = ((2, 4, 5), (4, 2, 5), (8, 1, 5), (1, 8, 5), (1, 4, 5), (2, 2, 5), (4, 1, 5),
         (2, 4, 3), (4, 2, 3), (8, 1, 3), (1, 8, 3), (1, 4, 3), (2, 2, 3), (4, 1, 3))          # (WVM, WVN, WN): dispatch_tile
S2D_TILES = ((2, 4, 2), (4, 2, 2), (2, 2, 2), (4, 1, 2), (1, 4, 2), (4, 1, 1), (2, 2, 1))      # (WVM, WVN, WN): kS2c
GROUP_TILES = ((4, 1, 5), (2, 2, 5), (4, 1, 3), (2, 2, 3))                                     # (WVM, WVN, WN): kCands of conv_group.hip

# ---- the search box (all three families)
BOX_NI = (1, 2, 3, 4, 8, 16, 32, 64)
BOX_CIN = (8, 16, 24, 40, 64, 136)
BOX_COUT = (8, 24, 40, 72, 136, 264)
# the model's pyramid at the 256 x 320 and 384 x 640 canvases (canvas, then strides 2 .. 32), and the small / wide / odd maps
BOX_MAPS = ((256, 320), (128, 160), (64, 80), (32, 40), (16, 20), (8, 10), (384, 640), (192, 320), (96, 160), (48, 80), (24, 40), (12, 20),
            (4, 6), (6, 4), (4, 10), (2, 14), (3, 30), (4, 640), (8, 320), (2, 96), (7, 10))
# the stride-2 input gradient also on every map less one row and one column (odd Hi, odd Wi: the last row / column has no odd neighbour)
S2D_MAPS = BOX_MAPS + tuple((h - 1, w - 1) for h, w in BOX_MAPS if h > 1)
BOX_CAP = 32 << 20          # floats of x and of y, each


def out_size(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def fwd_symbol(stride, op, vec, cand, lm=0):
    """op: 'f32' (three terms), 'int' (one term, fp32), 'planes'"""
    wvm, wvn, wn = TILES[cand]
    xt = 3 if op == 'f32' else 1
    nit = 2 if (wvm * wvn == 4 or xt == 1) else 1          # staging items per thread: N4 = 2, N8 = 2 with one term, else 1
    return f'conv_fwd_mfma_kernel<9, {stride}, {xt}, 1, {wn}, {wvm}, {wvn}, 16, {vec}, {nit}, {"true" if op == "planes" else "false"}, {lm}>'


def s2d_symbol(cand, vec):
    wvm, wvn, wn = S2D_TILES[cand]
    return f'conv_dgrad_s2c_kernel<{wn}, {wvm}, {wvn}, {vec}>'


def group_symbol(cand):
    wvm, wvn, wn = GROUP_TILES[cand]
    return f'conv3x3_group_kernel<3, {wn}, {wvm}, {wvn}, 2, 0, ConvGeomCore>'


def _plan_type():
    from eas_snn_amd import _lib
    return _lib.EasConvPlan


def fwd_plan(lib, shape, stride, x_terms, _out=[]):
    """(status, EasConvPlan) of eas_conv_fwd_plan; the plan object is reused by the next call"""
    if not _out:
        _out.append(_plan_type()())
    NI, Cin, Cout, H, W = shape
    return lib.eas_conv_fwd_plan(NI, Cin, Cout, H, W, 3, stride, x_terms, C.byref(_out[0])), _out[0]


def fwd_key(shape, stride, terms, p):
    Ho = out_size(shape[3], shape[4], stride)[0]
    return (stride, terms, p.vec, p.cand, p.single, p.parts, int(p.nseg > 1), int((shape[0] * Ho) % p.RT != 0))


def fwd_edges(shape, stride, p):
    """the edges of the issue's list this launch meets (names as in the comments of CASES)"""
    NI, Cin, Cout, H, W = shape
    Ho, Wo = out_size(H, W, stride)
    wvm = TILES[p.cand][0]
    e = set()
    if Cin == 8: e.add('cin8')                                          # one k-step with an empty upper half
    if Cin % 16 == 8 and Cin > 8: e.add('half')                         # half-empty last k-step
    if Cin > 32: e.add('3chunks')                                       # at least 3 channel chunks
    if Cout % 32: e.add('ragco')                                        # ragged last 32-channel tile
    if (wvm - 1) * 32 < Cout <= wvm * 32 - 8 and wvm > 1: e.add('idle')     # the block's upper wave row short of channels
    if ((Cout + 31) // 32) % wvm: e.add('norow')                        # wave rows of the last block row without any M-tile
    if p.nseg > 1: e.add('nseg')
    if p.RT < Ho: e.add('inimg')                                        # a tile inside an image
    if (NI * Ho) % p.RT: e.add('short')                                 # last tile short of rows
    if (p.RT * (Wo // p.parts)) % 32: e.add('pix32')                    # tile pixels no multiple of 32
    if stride == 2 and Ho % 2: e.add('oddHo')
    if H % 2: e.add('oddHi')
    if W % 4 == 2: e.add('vec2')
    e.add('1buf' if Cin <= 16 else ('single' if p.single else '2buf'))
    if p.parts > 1: e.add(f'parts{p.parts}')
    return frozenset(e)


def fwd_box():
    """(shape, stride) of the forward search box"""
    for s in (1, 2):
        for H, W in BOX_MAPS:
            Ho, Wo = out_size(H, W, s)
            for NI in BOX_NI:
                for Cin in BOX_CIN:
                    if NI * Cin * H * W > BOX_CAP:
                        continue
                    for Cout in BOX_COUT:
                        if NI * Cout * Ho * Wo <= BOX_CAP:
                            yield (NI, Cin, Cout, H, W), s


def s2d_plan(lib, shape, _out=[]):
    if not _out:
        _out.append(_plan_type()())
    return lib.eas_conv_dgrad_s2_plan(*shape, C.byref(_out[0])), _out[0]


def s2d_key(shape, p):
    Ho = out_size(shape[3], shape[4], 2)[0]
    return (p.cand, p.vec, int(p.bpi > 1), int(p.nseg > 1), int(p.bpi > 1 and Ho % p.RT != 0))


def s2d_edges(shape, p):
    NI, Cin, Cout, H, W = shape
    wvm = S2D_TILES[p.cand][0]
    e = set()
    if H % 2: e.add('oddHi')
    e.add('oddWi' if W % 2 else 'evenWi')                               # odd: 4-byte stores, no odd neighbour; even: the 8-byte pair stores
    if ((Cin + 31) // 32) % wvm: e.add('idle')                          # wave rows of the last block row without input channels
    if Cout == 8: e.add('co8')                                          # one k-step, one buffer
    if Cout == 40: e.add('co40')                                        # three k-steps, the last half empty
    return frozenset(e)


def s2d_box():
    for H, W in S2D_MAPS:
        for NI in BOX_NI:
            for Cin in BOX_CIN:
                if NI * Cin * H * W > BOX_CAP:
                    continue
                for Cout in BOX_COUT:
                    yield (NI, Cin, Cout, H, W)


def group_plan(lib, probs):
    """(status, [EasConvPlan]) of eas_conv_fwd_group_tile_plan for [(NI, Cin, Cout, H, W)]"""
    from eas_snn_amd import _lib
    n = len(probs)
    arr = (_lib.EasConvProblem * n)()
    for q, (NI, Cin, Cout, H, W) in zip(arr, probs):
        q.NI, q.Cin, q.Cout, q.Hi, q.Wi = NI, Cin, Cout, H, W
    out = (_lib.EasConvPlan * n)()
    return lib.eas_conv_fwd_group_tile_plan(arr, n, 3, 3, out), list(out)


# ------------------------------------------------------------------------------------------------ forward
# ((S, terms, VEC, candidate, single, parts, nseg > 1, ragged), (NI, Cin, Cout, H, W)): for every key the box reaches, the smallest box
# shape (x + y floats; among shapes up to twice that, the one that meets most edges), and further rows where a tile had not yet met an
# edge the box lets it meet.  The comment names the edges of fwd_edges the row meets: cin8 / half / 3chunks (Cin = 8, a half-empty last
# k-step, three or more channel chunks), ragco (Cout % 32 != 0), idle ((WVM - 1) * 32 < Cout <= WVM * 32 - 8), norow (wave rows without
# any M-tile in the last block row), nseg (whole images per tile), inimg (RT < Ho), short (NI * Ho % RT != 0), pix32 (tile pixels no
# multiple of 32), oddHo / oddHi, vec2 (Wi % 4 == 2), 1buf / 2buf / single, parts2 / parts4.  Eight column parts: not in the box.
CASES = [
    ((1, 1, 2, 11, 0, 1, 1, 0), (3, 8, 8, 3, 30)),  # 1buf cin8 nseg oddHi pix32 ragco vec2
    ((1, 1, 2, 11, 0, 1, 1, 1), (1, 8, 8, 4, 6)),  # 1buf cin8 nseg pix32 ragco short vec2
    ((1, 1, 2, 12, 0, 1, 1, 0), (2, 40, 40, 7, 10)),  # 2buf 3chunks half idle nseg oddHi pix32 ragco vec2
    ((1, 1, 2, 12, 0, 1, 1, 1), (1, 40, 40, 2, 14)),  # 2buf 3chunks half idle nseg pix32 ragco short vec2
    ((1, 1, 2, 13, 0, 1, 0, 0), (1, 40, 136, 7, 10)),  # 2buf 3chunks half norow oddHi pix32 ragco vec2
    ((1, 1, 2, 13, 0, 1, 1, 0), (2, 40, 136, 4, 10)),  # 2buf 3chunks half norow nseg pix32 ragco vec2
    ((1, 1, 2, 13, 0, 1, 1, 1), (1, 40, 136, 2, 14)),  # 2buf 3chunks half norow nseg pix32 ragco short vec2
    ((1, 1, 4, 0, 0, 1, 0, 0), (8, 8, 264, 4, 640)),  # 1buf cin8 inimg norow ragco
    ((1, 1, 4, 0, 0, 1, 0, 0), (8, 40, 264, 4, 640)),  # 2buf 3chunks half inimg norow ragco
    ((1, 1, 4, 3, 0, 1, 0, 0), (3, 8, 8, 192, 320)),  # 1buf cin8 inimg ragco
    ((1, 1, 4, 3, 0, 1, 0, 0), (3, 40, 8, 192, 320)),  # 2buf 3chunks half inimg ragco
    ((1, 1, 4, 4, 0, 1, 0, 0), (3, 40, 72, 96, 160)),  # 2buf 3chunks half inimg ragco
    ((1, 1, 4, 4, 0, 1, 0, 0), (8, 8, 8, 96, 160)),  # 1buf cin8 inimg ragco
    ((1, 1, 4, 5, 0, 1, 0, 0), (3, 8, 40, 96, 160)),  # 1buf cin8 idle inimg ragco
    ((1, 1, 4, 5, 0, 1, 0, 0), (4, 40, 264, 8, 320)),  # 2buf 3chunks half inimg norow ragco
    ((1, 1, 4, 6, 0, 1, 0, 0), (32, 8, 264, 12, 20)),  # 1buf cin8 inimg norow pix32 ragco
    ((1, 1, 4, 6, 0, 1, 0, 0), (32, 40, 264, 12, 20)),  # 2buf 3chunks half inimg norow pix32 ragco
    ((1, 1, 4, 10, 0, 1, 0, 0), (1, 8, 8, 4, 640)),  # 1buf cin8 inimg ragco
    ((1, 1, 4, 11, 0, 1, 0, 0), (1, 8, 8, 12, 20)),  # 1buf cin8 pix32 ragco
    ((1, 1, 4, 11, 0, 1, 1, 0), (16, 8, 8, 6, 4)),  # 1buf cin8 nseg ragco
    ((1, 1, 4, 11, 0, 1, 1, 1), (1, 8, 8, 6, 4)),  # 1buf cin8 nseg ragco short
    ((1, 1, 4, 12, 0, 1, 0, 0), (1, 8, 40, 12, 20)),  # 1buf cin8 idle inimg pix32 ragco
    ((1, 1, 4, 12, 0, 1, 1, 0), (8, 40, 40, 6, 4)),  # 2buf 3chunks half idle nseg ragco
    ((1, 1, 4, 12, 0, 1, 1, 1), (1, 40, 40, 6, 4)),  # 2buf 3chunks half idle nseg ragco short
    ((1, 1, 4, 13, 0, 1, 0, 0), (1, 40, 136, 12, 20)),  # 2buf 3chunks half inimg norow pix32 ragco
    ((1, 1, 4, 13, 0, 1, 1, 0), (4, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg ragco
    ((1, 1, 4, 13, 0, 1, 1, 1), (1, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg ragco short
    ((1, 3, 2, 11, 0, 1, 1, 0), (3, 8, 8, 3, 30)),  # 1buf cin8 nseg oddHi pix32 ragco vec2
    ((1, 3, 2, 11, 0, 1, 1, 1), (1, 8, 8, 4, 6)),  # 1buf cin8 nseg pix32 ragco short vec2
    ((1, 3, 2, 12, 0, 1, 1, 0), (2, 40, 40, 7, 10)),  # 2buf 3chunks half idle nseg oddHi pix32 ragco vec2
    ((1, 3, 2, 12, 0, 1, 1, 1), (1, 8, 72, 4, 6)),  # 1buf cin8 norow nseg ragco short vec2
    ((1, 3, 2, 12, 0, 1, 1, 1), (1, 40, 40, 2, 14)),  # 2buf 3chunks half idle nseg pix32 ragco short vec2
    ((1, 3, 2, 13, 0, 1, 0, 0), (1, 40, 136, 7, 10)),  # 2buf 3chunks half norow oddHi pix32 ragco vec2
    ((1, 3, 2, 13, 0, 1, 1, 0), (2, 40, 136, 4, 10)),  # 2buf 3chunks half norow nseg pix32 ragco vec2
    ((1, 3, 2, 13, 0, 1, 1, 1), (1, 8, 136, 4, 6)),  # 1buf cin8 norow nseg ragco short vec2
    ((1, 3, 2, 13, 0, 1, 1, 1), (1, 40, 136, 2, 14)),  # 2buf 3chunks half norow nseg pix32 ragco short vec2
    ((1, 3, 4, 0, 0, 1, 0, 0), (3, 136, 72, 96, 160)),  # 2buf 3chunks half inimg norow ragco
    ((1, 3, 4, 0, 0, 2, 0, 0), (1, 136, 72, 192, 320)),  # 2buf 3chunks half inimg norow parts2 ragco
    ((1, 3, 4, 0, 0, 4, 0, 0), (1, 136, 40, 384, 640)),  # 2buf 3chunks half idle inimg parts4 ragco
    ((1, 3, 4, 0, 1, 1, 0, 0), (64, 40, 136, 24, 40)),  # 3chunks half inimg norow ragco single
    ((1, 3, 4, 1, 0, 1, 0, 0), (2, 136, 136, 96, 160)),  # 2buf 3chunks half inimg norow ragco
    ((1, 3, 4, 1, 0, 1, 0, 0), (8, 8, 264, 8, 320)),  # 1buf cin8 inimg norow ragco
    ((1, 3, 4, 1, 0, 2, 0, 0), (16, 136, 136, 8, 320)),  # 2buf 3chunks half inimg norow parts2 ragco
    ((1, 3, 4, 1, 0, 4, 0, 0), (16, 136, 136, 4, 640)),  # 2buf 3chunks half inimg norow parts4 ragco
    ((1, 3, 4, 1, 1, 1, 0, 0), (3, 40, 136, 128, 160)),  # 3chunks half inimg norow ragco single
    ((1, 3, 4, 1, 1, 2, 0, 0), (1, 40, 136, 192, 320)),  # 3chunks half inimg norow parts2 ragco single
    ((1, 3, 4, 1, 1, 4, 0, 0), (32, 40, 136, 4, 640)),  # 3chunks half inimg norow parts4 ragco single
    ((1, 3, 4, 2, 0, 1, 0, 0), (1, 136, 264, 128, 160)),  # 2buf 3chunks half inimg norow ragco
    ((1, 3, 4, 2, 0, 2, 0, 0), (8, 136, 264, 8, 320)),  # 2buf 3chunks half inimg norow parts2 ragco
    ((1, 3, 4, 2, 0, 4, 0, 0), (8, 136, 264, 4, 640)),  # 2buf 3chunks half inimg norow parts4 ragco
    ((1, 3, 4, 2, 1, 1, 0, 0), (2, 40, 264, 128, 160)),  # 3chunks half inimg norow ragco single
    ((1, 3, 4, 2, 1, 2, 0, 0), (16, 40, 264, 8, 320)),  # 3chunks half inimg norow parts2 ragco single
    ((1, 3, 4, 2, 1, 4, 0, 0), (16, 40, 264, 4, 640)),  # 3chunks half inimg norow parts4 ragco single
    ((1, 3, 4, 4, 0, 1, 0, 0), (64, 8, 8, 48, 80)),  # 1buf cin8 inimg ragco
    ((1, 3, 4, 5, 0, 1, 0, 0), (64, 40, 72, 24, 40)),  # 2buf 3chunks half inimg norow ragco
    ((1, 3, 4, 6, 0, 1, 0, 0), (64, 40, 264, 12, 20)),  # 2buf 3chunks half inimg norow pix32 ragco
    ((1, 3, 4, 7, 0, 1, 0, 0), (1, 8, 40, 192, 320)),  # 1buf cin8 idle inimg ragco
    ((1, 3, 4, 7, 0, 1, 0, 0), (2, 40, 72, 96, 160)),  # 2buf 3chunks half inimg norow ragco
    ((1, 3, 4, 7, 0, 2, 0, 0), (16, 40, 72, 8, 320)),  # 2buf 3chunks half inimg norow parts2 ragco
    ((1, 3, 4, 7, 0, 4, 0, 0), (16, 40, 72, 4, 640)),  # 2buf 3chunks half inimg norow parts4 ragco
    ((1, 3, 4, 7, 1, 1, 0, 0), (3, 40, 72, 128, 160)),  # 3chunks half inimg norow ragco single
    ((1, 3, 4, 7, 1, 2, 0, 0), (1, 40, 72, 192, 320)),  # 3chunks half inimg norow parts2 ragco single
    ((1, 3, 4, 7, 1, 4, 0, 0), (32, 40, 72, 4, 640)),  # 3chunks half inimg norow parts4 ragco single
    ((1, 3, 4, 8, 0, 1, 0, 0), (1, 40, 136, 128, 160)),  # 2buf 3chunks half inimg norow ragco
    ((1, 3, 4, 8, 0, 2, 0, 0), (4, 40, 264, 8, 320)),  # 2buf 3chunks half inimg norow parts2 ragco
    ((1, 3, 4, 8, 0, 4, 0, 0), (4, 40, 264, 4, 640)),  # 2buf 3chunks half inimg norow parts4 ragco
    ((1, 3, 4, 8, 1, 1, 0, 0), (1, 40, 264, 128, 160)),  # 3chunks half inimg norow ragco single
    ((1, 3, 4, 8, 1, 2, 0, 0), (8, 40, 264, 8, 320)),  # 3chunks half inimg norow parts2 ragco single
    ((1, 3, 4, 8, 1, 4, 0, 0), (8, 40, 264, 4, 640)),  # 3chunks half inimg norow parts4 ragco single
    ((1, 3, 4, 10, 0, 1, 0, 0), (8, 40, 136, 48, 80)),  # 2buf 3chunks half inimg ragco
    ((1, 3, 4, 10, 0, 1, 1, 1), (64, 8, 264, 12, 20)),  # 1buf cin8 nseg pix32 ragco short
    ((1, 3, 4, 10, 0, 2, 0, 0), (2, 40, 8, 192, 320)),  # 2buf 3chunks half inimg parts2 ragco
    ((1, 3, 4, 10, 0, 4, 0, 0), (1, 40, 8, 384, 640)),  # 2buf 3chunks half inimg parts4 ragco
    ((1, 3, 4, 10, 1, 1, 0, 0), (16, 40, 136, 48, 80)),  # 3chunks half inimg ragco single
    ((1, 3, 4, 11, 0, 1, 0, 0), (1, 8, 8, 12, 20)),  # 1buf cin8 pix32 ragco
    ((1, 3, 4, 11, 0, 1, 1, 0), (16, 8, 8, 6, 4)),  # 1buf cin8 nseg ragco
    ((1, 3, 4, 11, 0, 1, 1, 1), (1, 8, 8, 6, 4)),  # 1buf cin8 nseg ragco short
    ((1, 3, 4, 11, 0, 2, 0, 0), (1, 8, 8, 4, 640)),  # 1buf cin8 inimg parts2 ragco
    ((1, 3, 4, 11, 0, 4, 0, 0), (1, 40, 8, 4, 640)),  # 2buf 3chunks half inimg parts4 ragco
    ((1, 3, 4, 11, 1, 1, 0, 0), (3, 40, 72, 96, 160)),  # 3chunks half inimg ragco single
    ((1, 3, 4, 11, 1, 2, 0, 0), (2, 40, 8, 256, 320)),  # 3chunks half inimg parts2 ragco single
    ((1, 3, 4, 11, 1, 4, 0, 0), (64, 40, 8, 4, 640)),  # 3chunks half inimg parts4 ragco single
    ((1, 3, 4, 12, 0, 1, 0, 0), (1, 8, 40, 12, 20)),  # 1buf cin8 idle inimg pix32 ragco
    ((1, 3, 4, 12, 0, 1, 1, 0), (8, 40, 40, 6, 4)),  # 2buf 3chunks half idle nseg ragco
    ((1, 3, 4, 12, 0, 1, 1, 1), (1, 40, 40, 6, 4)),  # 2buf 3chunks half idle nseg ragco short
    ((1, 3, 4, 12, 0, 2, 0, 0), (1, 40, 40, 8, 320)),  # 2buf 3chunks half idle inimg parts2 ragco
    ((1, 3, 4, 12, 0, 4, 0, 0), (1, 40, 40, 4, 640)),  # 2buf 3chunks half idle inimg parts4 ragco
    ((1, 3, 4, 13, 0, 1, 0, 0), (1, 40, 136, 12, 20)),  # 2buf 3chunks half inimg norow pix32 ragco
    ((1, 3, 4, 13, 0, 1, 1, 0), (4, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg ragco
    ((1, 3, 4, 13, 0, 1, 1, 1), (1, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg ragco short
    ((2, 1, 2, 11, 0, 1, 1, 0), (2, 8, 8, 3, 30)),  # 1buf cin8 nseg oddHi pix32 ragco vec2
    ((2, 1, 2, 11, 0, 1, 1, 1), (1, 8, 8, 2, 14)),  # 1buf cin8 nseg oddHo pix32 ragco short vec2
    ((2, 1, 2, 12, 0, 1, 1, 0), (2, 8, 40, 3, 30)),  # 1buf cin8 idle nseg oddHi pix32 ragco vec2
    ((2, 1, 2, 12, 0, 1, 1, 1), (1, 8, 40, 2, 14)),  # 1buf cin8 idle nseg oddHo pix32 ragco short vec2
    ((2, 1, 2, 13, 0, 1, 1, 0), (8, 40, 136, 2, 14)),  # 2buf 3chunks half norow nseg oddHo pix32 ragco vec2
    ((2, 1, 2, 13, 0, 1, 1, 1), (1, 8, 136, 2, 14)),  # 1buf cin8 norow nseg oddHo pix32 ragco short vec2
    ((2, 1, 4, 0, 0, 1, 0, 0), (64, 8, 72, 48, 80)),  # 1buf cin8 inimg norow ragco
    ((2, 1, 4, 0, 0, 1, 0, 0), (64, 40, 72, 48, 80)),  # 2buf 3chunks half inimg norow ragco
    ((2, 1, 4, 1, 0, 1, 0, 0), (32, 8, 264, 4, 640)),  # 1buf cin8 inimg norow ragco
    ((2, 1, 4, 1, 0, 1, 0, 0), (32, 40, 264, 4, 640)),  # 2buf 3chunks half inimg norow ragco
    ((2, 1, 4, 6, 0, 1, 0, 0), (32, 40, 264, 24, 40)),  # 2buf 3chunks half inimg norow pix32 ragco
    ((2, 1, 4, 7, 0, 1, 0, 0), (1, 8, 40, 4, 640)),  # 1buf cin8 idle inimg ragco
    ((2, 1, 4, 7, 0, 1, 0, 0), (1, 40, 72, 4, 640)),  # 2buf 3chunks half inimg norow ragco
    ((2, 1, 4, 10, 0, 1, 0, 0), (1, 8, 8, 4, 640)),  # 1buf cin8 inimg ragco
    ((2, 1, 4, 10, 0, 1, 0, 0), (1, 40, 8, 4, 640)),  # 2buf 3chunks half inimg ragco
    ((2, 1, 4, 11, 0, 1, 0, 0), (1, 8, 8, 24, 40)),  # 1buf cin8 pix32 ragco
    ((2, 1, 4, 11, 0, 1, 1, 0), (3, 8, 8, 2, 96)),  # 1buf cin8 nseg oddHo pix32 ragco
    ((2, 1, 4, 11, 0, 1, 1, 1), (1, 8, 8, 6, 4)),  # 1buf cin8 nseg oddHo pix32 ragco short
    ((2, 1, 4, 12, 0, 1, 0, 0), (1, 8, 40, 24, 40)),  # 1buf cin8 idle inimg pix32 ragco
    ((2, 1, 4, 12, 0, 1, 1, 0), (3, 8, 40, 2, 96)),  # 1buf cin8 idle nseg oddHo pix32 ragco
    ((2, 1, 4, 12, 0, 1, 1, 1), (1, 8, 40, 6, 4)),  # 1buf cin8 idle nseg oddHo ragco short
    ((2, 1, 4, 13, 0, 1, 0, 0), (1, 40, 136, 12, 20)),  # 2buf 3chunks half norow pix32 ragco
    ((2, 1, 4, 13, 0, 1, 1, 0), (16, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg oddHo ragco
    ((2, 1, 4, 13, 0, 1, 1, 1), (1, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg oddHo ragco short
    ((2, 3, 2, 11, 0, 1, 1, 0), (2, 8, 8, 3, 30)),  # 1buf cin8 nseg oddHi pix32 ragco vec2
    ((2, 3, 2, 11, 0, 1, 1, 1), (1, 8, 8, 2, 14)),  # 1buf cin8 nseg oddHo pix32 ragco short vec2
    ((2, 3, 2, 12, 0, 1, 1, 0), (2, 8, 40, 3, 30)),  # 1buf cin8 idle nseg oddHi pix32 ragco vec2
    ((2, 3, 2, 12, 0, 1, 1, 1), (1, 8, 40, 2, 14)),  # 1buf cin8 idle nseg oddHo pix32 ragco short vec2
    ((2, 3, 2, 13, 0, 1, 1, 0), (8, 40, 136, 2, 14)),  # 2buf 3chunks half norow nseg oddHo pix32 ragco vec2
    ((2, 3, 2, 13, 0, 1, 1, 1), (1, 8, 136, 2, 14)),  # 1buf cin8 norow nseg oddHo pix32 ragco short vec2
    ((2, 3, 2, 13, 0, 1, 1, 1), (1, 8, 136, 7, 10)),  # 1buf cin8 norow nseg oddHi pix32 ragco short vec2
    ((2, 3, 4, 2, 0, 1, 0, 0), (64, 64, 264, 24, 40)),  # 2buf 3chunks inimg norow pix32 ragco
    ((2, 3, 4, 2, 0, 2, 0, 0), (32, 8, 264, 4, 640)),  # 1buf cin8 inimg norow parts2 ragco
    ((2, 3, 4, 2, 0, 4, 0, 0), (32, 136, 264, 4, 640)),  # 2buf 3chunks half norow parts4 ragco
    ((2, 3, 4, 2, 1, 1, 0, 0), (8, 40, 264, 96, 160)),  # 3chunks half inimg norow ragco single
    ((2, 3, 4, 2, 1, 2, 0, 0), (2, 40, 264, 192, 320)),  # 3chunks half inimg norow parts2 ragco single
    ((2, 3, 4, 2, 1, 4, 0, 0), (1, 40, 264, 384, 640)),  # 3chunks half inimg norow parts4 ragco single
    ((2, 3, 4, 6, 0, 1, 0, 0), (64, 8, 264, 24, 40)),  # 1buf cin8 inimg norow pix32 ragco
    ((2, 3, 4, 8, 0, 1, 0, 0), (1, 8, 136, 192, 320)),  # 1buf cin8 inimg norow ragco
    ((2, 3, 4, 8, 0, 1, 0, 0), (3, 40, 136, 128, 160)),  # 2buf 3chunks half inimg norow ragco
    ((2, 3, 4, 8, 0, 2, 0, 0), (1, 40, 136, 192, 320)),  # 2buf 3chunks half inimg norow parts2 ragco
    ((2, 3, 4, 8, 0, 4, 0, 0), (32, 40, 136, 4, 640)),  # 2buf 3chunks half norow parts4 ragco
    ((2, 3, 4, 8, 1, 1, 0, 0), (64, 40, 264, 24, 40)),  # 3chunks half inimg norow pix32 ragco single
    ((2, 3, 4, 8, 1, 2, 0, 0), (2, 40, 136, 192, 320)),  # 3chunks half inimg norow parts2 ragco single
    ((2, 3, 4, 8, 1, 4, 0, 0), (1, 40, 136, 384, 640)),  # 3chunks half inimg norow parts4 ragco single
    ((2, 3, 4, 9, 0, 1, 0, 0), (2, 40, 264, 128, 160)),  # 2buf 3chunks half inimg norow pix32 ragco
    ((2, 3, 4, 9, 0, 2, 0, 0), (16, 40, 264, 8, 320)),  # 2buf 3chunks half inimg norow parts2 pix32 ragco
    ((2, 3, 4, 9, 0, 4, 0, 0), (16, 40, 264, 4, 640)),  # 2buf 3chunks half inimg norow parts4 pix32 ragco
    ((2, 3, 4, 9, 1, 1, 0, 0), (4, 40, 264, 128, 160)),  # 3chunks half inimg norow pix32 ragco single
    ((2, 3, 4, 9, 1, 2, 0, 0), (1, 40, 264, 256, 320)),  # 3chunks half inimg norow parts2 pix32 ragco single
    ((2, 3, 4, 9, 1, 4, 0, 0), (32, 40, 264, 4, 640)),  # 3chunks half inimg norow parts4 pix32 ragco single
    ((2, 3, 4, 11, 0, 1, 0, 0), (1, 8, 8, 24, 40)),  # 1buf cin8 pix32 ragco
    ((2, 3, 4, 11, 0, 1, 1, 0), (3, 8, 8, 2, 96)),  # 1buf cin8 nseg oddHo pix32 ragco
    ((2, 3, 4, 11, 0, 1, 1, 1), (1, 8, 8, 6, 4)),  # 1buf cin8 nseg oddHo pix32 ragco short
    ((2, 3, 4, 11, 0, 2, 0, 0), (1, 8, 8, 4, 640)),  # 1buf cin8 inimg parts2 ragco
    ((2, 3, 4, 11, 0, 4, 0, 0), (1, 40, 8, 4, 640)),  # 2buf 3chunks half parts4 ragco
    ((2, 3, 4, 11, 1, 1, 0, 0), (16, 40, 8, 96, 160)),  # 3chunks half inimg ragco single
    ((2, 3, 4, 11, 1, 2, 0, 0), (3, 40, 8, 192, 320)),  # 3chunks half inimg parts2 ragco single
    ((2, 3, 4, 11, 1, 4, 0, 0), (1, 40, 8, 384, 640)),  # 3chunks half inimg parts4 ragco single
    ((2, 3, 4, 12, 0, 1, 0, 0), (1, 8, 40, 24, 40)),  # 1buf cin8 idle inimg pix32 ragco
    ((2, 3, 4, 12, 0, 1, 1, 0), (3, 8, 40, 2, 96)),  # 1buf cin8 idle nseg oddHo pix32 ragco
    ((2, 3, 4, 12, 0, 1, 1, 1), (1, 24, 40, 6, 4)),  # 2buf half idle nseg oddHo pix32 ragco short
    ((2, 3, 4, 12, 0, 2, 0, 0), (1, 8, 40, 4, 640)),  # 1buf cin8 idle inimg parts2 ragco
    ((2, 3, 4, 12, 0, 4, 0, 0), (1, 40, 40, 4, 640)),  # 2buf 3chunks half idle parts4 ragco
    ((2, 3, 4, 12, 1, 1, 0, 0), (3, 40, 264, 128, 160)),  # 3chunks half inimg norow ragco single
    ((2, 3, 4, 12, 1, 2, 0, 0), (1, 40, 264, 192, 320)),  # 3chunks half inimg norow parts2 ragco single
    ((2, 3, 4, 12, 1, 4, 0, 0), (1, 40, 40, 384, 640)),  # 3chunks half idle inimg parts4 ragco single
    ((2, 3, 4, 13, 0, 1, 0, 0), (1, 40, 136, 12, 20)),  # 2buf 3chunks half norow pix32 ragco
    ((2, 3, 4, 13, 0, 1, 1, 0), (16, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg oddHo ragco
    ((2, 3, 4, 13, 0, 1, 1, 1), (1, 40, 136, 6, 4)),  # 2buf 3chunks half norow nseg oddHo ragco short
    ((2, 3, 4, 13, 0, 2, 0, 0), (1, 40, 136, 8, 320)),  # 2buf 3chunks half inimg norow parts2 pix32 ragco
    ((2, 3, 4, 13, 0, 4, 0, 0), (1, 40, 136, 4, 640)),  # 2buf 3chunks half inimg norow parts4 pix32 ragco
]

# Compiled LM = 0 instances (S, terms, VEC, candidate) the box never reaches -> (reason, ratio).  terms 1 names two instances (fp32 and
# planes).  The reasons are read from dispatch_tile's rule: cost = rounds of 256 CUs x round factor x conv_block_time(WN) with round
# factors 1.27 (one eight-wave block per CU), 1.2 (a pair of four-wave blocks whose patches fit the LDS twice, more than 256 blocks), 1.0
# (lone four-wave blocks) and conv_block_time 1.0 for WN = 5, 0.72 (three terms) / 0.956 (one term: the 450-cycle floor) for WN = 3; a
# candidate needs Cout > (WVM - 1) * 32.  ratio: a line-by-line restatement of the rule, which agreed with the planner on every geometry
# of the box, gave the candidate's cost / the winner's cost wherever the candidate had channels and fitted -- never below this figure, so
# none of them ever came as close as a tie.  The walk asserts the box indeed never reaches them: a change of the rule that makes one
# reachable fails there.
_R_VEC2 = ('VEC 2 runs on rows with Wi % 4 == 2; those of the box hold at most 90 pixels (3 x 30) x 64 images, which four-wave blocks with '
           '96-pixel wave tiles cover in one round of at most 256 blocks: the cheapest round of the table; ')
_R_PAIR = ('an eight-wave block (1.27 per round) against a pair of four-wave blocks of the same wave tiles (1.2): with one-term patches the '
           'pair fits the LDS wherever this tile has channels and fits')
LEFT_OUT = {}
for _s in (1, 2):
    for _t, _r5, _r58 in ((3, 1.389, 1.764), (1, 1.046, 1.328)):
        LEFT_OUT.update({(_s, _t, 2, _c): (_R_VEC2 + 'an eight-wave WN = 5 tile costs 1.27 x conv_block_time(5)', _r58) for _c in (0, 1, 2, 3)})
        LEFT_OUT.update({(_s, _t, 2, _c): (_R_VEC2 + 'a four-wave WN = 5 tile costs conv_block_time(5)', _r5) for _c in (4, 5, 6)})
        LEFT_OUT.update({(_s, _t, 2, _c): (_R_VEC2 + 'an eight-wave WN = 3 tile costs 1.27 x as much', 1.27) for _c in (7, 8, 9, 10)})
LEFT_OUT.update({(1, 1, 4, _c): (_R_PAIR, 1.058) for _c in (1, 2, 7, 8, 9)})
LEFT_OUT.update({
    (1, 3, 4, 3): ('(1,8,5), three terms: one eight-wave block of WN = 5 per CU; the four-wave WN = 3 tiles (11, 12, 13) or (2,4,3) cover every '
                   'box geometry in no more rounds at 0.72 of its block time', 1.389),
    (1, 3, 4, 9): ('(8,1,3), stride 1: needs Cout > 224 (Cout 264 in the box: 9 M-tiles, 7 of its 16 wave rows idle); (4,1,3) pairs cost 1.2 '
                   'against its 1.27 for the same rounds', 1.058),
    (2, 1, 4, 2): (_R_PAIR, 1.058),
    (2, 1, 4, 3): ('(1,8,5), stride 2, one term: conv_block_time(5) against the 0.956 of the WN = 3 tiles, which need no more rounds', 1.046),
    (2, 1, 4, 4): ('(1,4,5), stride 2, one term: as (1,8,5); its 640-pixel tile stages four times the input pixels and does not fit the '
                   'staging slots on the wide rows', 1.046),
    (2, 1, 4, 5): ('(2,2,5), stride 2, one term: as (1,4,5); in 18 box geometries it ties with the winner and loses the tie on WVM or valid '
                   'pixels', 1.0),
    (2, 1, 4, 8): (_R_PAIR, 1.214),
    (2, 1, 4, 9): (_R_PAIR, 1.214),
    (2, 3, 4, 0): ('(2,4,5), stride 2, three terms: an eight-wave WN = 5 block; the WN = 3 tiles cost 0.72 of its block time in no more rounds', 1.47),
    (2, 3, 4, 1): ('(4,2,5), stride 2, three terms: as (2,4,5); closest where (4,1,3) pairs cost 1.2 against 1.27', 1.058),
    (2, 3, 4, 3): ('(1,8,5), stride 2, three terms: as (2,4,5)', 1.764),
    (2, 3, 4, 4): ('(1,4,5), stride 2, three terms: conv_block_time(5) against the 0.72 of (1,4,3) in the same rounds', 1.389),
    (2, 3, 4, 5): ('(2,2,5), stride 2, three terms: as (1,4,5), against (2,2,3)', 1.157),
    (2, 3, 4, 7): ('(2,4,3), stride 2, three terms: an eight-wave block against pairs of (2,2,3) / (4,1,3) blocks', 1.058),
    (2, 3, 4, 10): ('(1,8,3), stride 2, three terms: an eight-wave block against lone (1,4,3) / (2,2,3) blocks of the same rounds', 1.27)})

# ------------------------------------------------------------------------------------------------ stride-2 input gradient
# ((candidate, VEC, bpi > 1, nseg > 1, short), (NI, Cin, Cout, Hi, Wi)); edges of s2d_edges: oddHi / oddWi (last row / column without an
# odd neighbour, 4-byte stores), evenWi (the 8-byte pair stores), idle (wave rows without input channels), co8 (one k-step, one buffer),
# co40 (three k-steps, the last half empty)
S2D_CASES = [
    ((2, 2, 1, 0, 0), (1, 40, 8, 95, 159)),  # co8 oddHi oddWi
    ((2, 2, 1, 0, 0), (1, 40, 8, 96, 160)),  # co8 evenWi
    ((2, 2, 1, 0, 0), (1, 40, 40, 95, 159)),  # co40 oddHi oddWi
    ((2, 2, 1, 0, 1), (32, 136, 8, 31, 39)),  # co8 idle oddHi oddWi
    ((4, 1, 0, 1, 0), (1, 8, 8, 5, 3)),  # co8 oddHi oddWi
    ((4, 1, 0, 1, 0), (1, 8, 8, 6, 4)),  # co8 evenWi
    ((4, 1, 0, 1, 0), (1, 8, 40, 5, 3)),  # co40 oddHi oddWi
    ((4, 2, 1, 0, 0), (1, 8, 8, 31, 39)),  # co8 oddHi oddWi
    ((4, 4, 0, 0, 0), (1, 8, 8, 23, 39)),  # co8 oddHi oddWi
    ((4, 4, 0, 1, 0), (1, 8, 8, 1, 95)),  # co8 oddHi oddWi
    ((4, 4, 1, 0, 0), (1, 8, 8, 7, 319)),  # co8 oddHi oddWi
    ((4, 4, 1, 0, 1), (1, 8, 8, 63, 79)),  # co8 oddHi oddWi
    ((5, 2, 0, 1, 0), (1, 136, 8, 5, 3)),  # co8 idle oddHi oddWi
    ((5, 2, 0, 1, 0), (1, 136, 8, 6, 4)),  # co8 evenWi idle
    ((5, 2, 0, 1, 0), (1, 136, 40, 5, 3)),  # co40 idle oddHi oddWi
    ((5, 2, 1, 0, 0), (1, 136, 8, 11, 19)),  # co8 idle oddHi oddWi
    ((5, 2, 1, 0, 1), (1, 136, 8, 15, 19)),  # co8 idle oddHi oddWi
    ((6, 2, 0, 0, 0), (1, 40, 8, 1, 95)),  # co8 oddHi oddWi
    ((6, 2, 0, 0, 0), (1, 136, 8, 1, 95)),  # co8 idle oddHi oddWi
    ((6, 2, 0, 1, 0), (1, 40, 8, 5, 3)),  # co8 oddHi oddWi
    ((6, 2, 0, 1, 0), (1, 40, 8, 6, 4)),  # co8 evenWi
    ((6, 2, 0, 1, 0), (1, 40, 40, 5, 3)),  # co40 oddHi oddWi
    ((6, 2, 1, 0, 0), (1, 40, 8, 15, 19)),  # co8 oddHi oddWi
    ((6, 2, 1, 0, 1), (1, 40, 8, 31, 39)),  # co8 oddHi oddWi
]

# (candidate, VEC) of conv_dgrad_s2c_kernel the box never reaches (dgrad_s2_plan: staging width 2 first, then 4 where Wo % 4 == 0, then 1 --
# the first whose items fit one per thread, four per thread for width 1; cost as above, the first candidate keeps a tie)
# (a restatement of the rule that agreed with the planner on every geometry of the box gave the figures)
_R_S2D_8W = ('eight-wave tile: wherever it has channels and fits, its staging width is 2 and a pair of four-wave blocks (1.2 per round) beats '
             'the one eight-wave block (1.27): cost at least 1.058 x the winner\'s')
_R_S2D_413 = ('(4,1,2): needs Cin > 96 (Cin 136 in the box); its staging width is always 2, and it costs at least 1.026 x the winner -- or, in '
              '24 box geometries, as much as an earlier candidate, which keeps a tie')
_R_S2D_VEC = ('staging width 2 fits this four-wave tile wherever the tile fits (at most 128 positions and their halo, two per item, against '
              '256 threads), so widths 4 and 1 are never asked')
S2D_LEFT_OUT = {(_c, _v): _R_S2D_8W for _c in (0, 1) for _v in (4, 2, 1)}
S2D_LEFT_OUT.update({(3, _v): _R_S2D_413 for _v in (4, 2, 1)})
S2D_LEFT_OUT.update({(_c, _v): _R_S2D_VEC for _c in (2, 5, 6) for _v in (4, 1)})

# ------------------------------------------------------------------------------------------------ grouped 3x3
# name -> (candidate in GROUP_TILES, [(NI, Cin, Cout, H, W)] x 3, staging width per problem): three maps and three Cin per group; 'c0' and
# 'c3' mix a VEC 4 and a VEC 2 problem (10- and 6-pixel rows); 'c3' has tiles of several whole images
GROUP_CASES = {
    'c0': (0, [(32, 8, 136, 32, 40), (32, 24, 136, 16, 20), (32, 40, 136, 8, 10)], (4, 4, 2)),
    'c1': (1, [(16, 8, 40, 64, 80), (16, 24, 72, 32, 40), (16, 40, 40, 16, 20)], (4, 4, 4)),
    'c2': (2, [(1, 8, 136, 64, 80), (1, 24, 136, 32, 40), (1, 40, 136, 16, 20)], (4, 4, 4)),
    'c3': (3, [(1, 8, 40, 8, 10), (1, 24, 72, 4, 6), (1, 40, 40, 6, 4)], (2, 2, 4))}

# geometries no tile takes: Cin % 8 != 0, an odd Wi, and rows too wide for any patch even in eight column parts
# (8192-pixel rows: an eighth of a row is 1024 pixels, more than any tile but (1,8,5), whose patch does not fit)
REFUSED = [(1, 12, 16, 8, 12, 1), (1, 8, 16, 8, 9, 1), (1, 8, 16, 8, 9, 2), (1, 64, 8, 4, 8192, 1), (1, 64, 8, 4, 8192, 2)]          # (NI, Cin, Cout, H, W, stride)
