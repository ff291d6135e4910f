"""Packed-W4 instantiations of the LDS-halo conv kernel (csrc/iconv.hip), host side: the weight stage's address
functions restated and enumerated (DMA side and fragment-read side agree slot for slot; no two lanes of a
32-lane half of a ds_read_b64 on one LDS bank), the C-ABI query, and the Python plumbing.  No GPU."""
import ctypes

import pytest
import torch

# tile id -> TH, TW, BN, CK, WNG (halo_conv_launch)
TILES = {90: (8, 16, 80, 128, 1), 91: (8, 8, 80, 128, 1), 92: (16, 16, 80, 64, 1), 93: (16, 16, 160, 64, 2)}


def _geom(tile):
    TH, TW, BN, CK, WNG = TILES[tile]
    wrow = CK // 2                      # bytes of a packed weight row of one channel chunk
    wlpp = wrow // 16                   # 16-byte DMA slots per row
    w_tap = BN * wrow
    pieces = (3 * w_tap + 1023) // 1024
    return dict(BN=BN, CK=CK, WNG=WNG, BM=TH * TW, wrow=wrow, wlpp=wlpp, w_tap=w_tap, pieces=pieces,
                ksplit=CK // 64, wpx=8 // (CK // 64) // WNG, wtn=BN // WNG)


def _wswz(wrow, row):
    """HaloGeom::wswz: the XOR term on the 16-byte slot index of a packed row."""
    return (row >> 2) & 3 if wrow == 64 else (row >> 3) & 1


def _dma_image(g):
    """LDS byte address of every 16-byte slot of a filter-row stage -> (tap, row, source byte offset in the row's
    packed chunk), as the kernel's per-lane DMA state lays it out: piece q of the stage goes to q * 1024, lane l
    of the wave writes 16 bytes at l * 16 (LDS-DMA is not a per-lane scatter), and the lane picks its SOURCE."""
    image, pad = {}, 0
    for q in range(g["pieces"]):
        for lane in range(64):
            L = q * 64 + lane
            s, rem = divmod(L, g["BN"] * g["wlpp"])
            row, slot = divmod(rem, g["wlpp"])
            if L >= 3 * g["BN"] * g["wlpp"]:
                pad += 1                     # reads the zero page
                continue
            image[L * 16] = (s, row, (slot ^ _wswz(g["wrow"], row)) << 4)
    return image, pad


def _read_addr(g, wid, tn, lane, s):
    """(byte address in the stage, row, source byte the lane expects) of fragment tn of tap s."""
    lrow, lkq = lane & 15, lane >> 4
    kg = wid // g["wpx"] if g["WNG"] == 1 else 0
    wn = 0 if g["WNG"] == 1 else wid // g["wpx"]
    row = wn * g["wtn"] + tn * 16 + lrow
    slot = kg * 2 + (lkq >> 1)
    addr = s * g["w_tap"] + row * g["wrow"] + ((slot ^ _wswz(g["wrow"], row)) << 4) + (lkq & 1) * 8
    return addr, row, kg * 32 + lkq * 8


@pytest.mark.parametrize("tile", sorted(TILES))
def test_w4_stage_dma_covers_every_slot_once_and_pads_to_whole_pieces(tile):
    g = _geom(tile)
    image, pad = _dma_image(g)
    want = {(s, row, c) for s in range(3) for row in range(g["BN"]) for c in range(0, g["wrow"], 16)}
    assert len(image) == len(want) and set(image.values()) == want
    assert (len(image) + pad) * 16 == g["pieces"] * 1024
    assert pad * 16 < 1024                                   # less than one piece of padding
    assert pad == {90: 0, 91: 0, 92: 32, 93: 0}[tile]        # 80 x 32 bytes x 3 taps = 7.5 pieces
    # the permutation stays inside a row: whole 16-byte slots move, never bytes across rows or taps
    for addr, (s, row, c) in image.items():
        assert addr // g["wrow"] == s * g["BN"] + row


@pytest.mark.parametrize("tile", sorted(TILES))
def test_w4_fragment_read_finds_what_the_dma_put_there_and_is_bank_conflict_free(tile):
    """ds_read_b64: served per 32-lane half, bank of byte address a = (a / 4) % 64, 8 bytes = two banks per lane.
    Every wave (both k-split groups / both channel groups), every fragment, every tap."""
    g = _geom(tile)
    image, _ = _dma_image(g)
    tn_count = g["wtn"] // 16
    worst = 0
    for wid in range(8):
        for s in range(3):
            for tn in range(tn_count):
                for half in range(2):
                    banks = {}
                    for lane in range(half * 32, half * 32 + 32):
                        addr, row, src = _read_addr(g, wid, tn, lane, s)
                        assert addr % 8 == 0                           # natural alignment of a 64-bit DS read
                        assert addr + 8 <= g["pieces"] * 1024
                        slot_addr = addr & ~15
                        ts, trow, tc = image[slot_addr]                # KeyError: a read of stage padding
                        assert (ts, trow) == (s, row)
                        assert tc + (addr & 15) == src, (tile, wid, tn, lane)
                        for b in ((addr // 4) % 64, (addr // 4 + 1) % 64):
                            banks.setdefault(b, set()).add(addr)
                    ways = max(len(v) for v in banks.values())
                    worst = max(worst, ways)
                    assert len(banks) == 64 and ways == 1, (tile, wid, s, tn, half, ways)
    assert worst == 1


@pytest.mark.parametrize("tile", sorted(TILES))
def test_w4_unswizzled_rows_would_conflict(tile):
    """The enumeration above is not vacuous: without the XOR term the same reads are 4-way (64-byte rows: 16 rows
    x 2 k-quarters land on 16 of the 64 banks ... of a 256-byte bank row that holds 4 rows) or 2-way (32-byte rows)."""
    g = _geom(tile)
    banks = {}
    for lane in range(32):
        lrow, lkq = lane & 15, lane >> 4
        addr = lrow * g["wrow"] + lkq * 8
        for b in ((addr // 4) % 64, (addr // 4 + 1) % 64):
            banks.setdefault(b, set()).add(addr)
    assert max(len(v) for v in banks.values()) == (4 if g["wrow"] == 64 else 2)


def test_w4_unpack_gives_sixteen_q_in_natural_k_order():
    """The fragment's 8 packed bytes -> four MFMA operand dwords: w & 0xF0F0F0F0, (w << 4) & 0xF0F0F0F0 per dword
    are the int8 values 16 * q[0..3], 16 * q[4..7] (pack_w4's layout), for the whole range [-8, 7]."""
    from mixdq_amd.nn.utils import pack_w4
    q = (torch.arange(64, dtype=torch.int32) % 16 - 8).to(torch.int8).reshape(4, 16)
    q[1] = q[1].flip(0)
    packed = pack_w4(q).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF     # [4, 2] dwords
    for r in range(4):
        regs = []
        for w in packed[r].tolist():
            regs += [w & 0xF0F0F0F0, (w << 4) & 0xF0F0F0F0]
        got = torch.tensor([(reg >> (8 * j)) & 0xFF for reg in regs for j in range(4)], dtype=torch.uint8).view(torch.int8)
        assert torch.equal(got.to(torch.int32), 16 * q[r].to(torch.int32))


def test_w4_resources_fit_the_cu():
    """LDS of the four instantiations (HaloGeom::SMEM restated): within 160 KiB, and tile 92 small enough for two
    workgroups per CU."""
    smem = {}
    for tile, (TH, TW, BN, CK, WNG) in TILES.items():
        g = _geom(tile)
        hp = (TH + 2) * (TW + 2)
        ppp = 1024 // CK
        h_ni = -(-(-(-hp // ppp)) // 8)
        main = 3 * g["pieces"] * 1024 + 2 * h_ni * 8 * 1024
        tm, tn = g["BM"] // g["wpx"] // 16, g["wtn"] // 16
        part = (g["ksplit"] - 1) * g["wpx"] * tm * tn * 4 * 64 * 4
        assert g["BM"] * (BN * 2 + 16) + part <= main          # the epilogue tile overlays the main buffers
        smem[tile] = main + 9 * BN * 4 + BN * 6
    assert smem == {90: 98592, 91: 82208, 92: 77088, 93: 101952}
    assert 2 * smem[92] <= 160 * 1024


def test_flags_query_is_declared_exported_and_keeps_the_w8_answers():
    from tests.test_cabi import declared_symbols
    from mixdq_amd.build import build
    assert "mixdq_conv_halo_select_flags" in declared_symbols()
    lib = ctypes.CDLL(build())
    old, new = lib.mixdq_conv_halo_select, lib.mixdq_conv_halo_select_flags
    old.argtypes, old.restype = [ctypes.c_int] * 9, ctypes.c_int
    new.argtypes, new.restype = [ctypes.c_int] * 10, ctypes.c_int
    lib.mixdq_abi_version.restype = ctypes.c_int
    assert lib.mixdq_abi_version() == 3                         # additions only
    W4, W2 = 2, 16
    shapes = [(1, 128, 128, 320, 320), (1, 64, 64, 640, 640), (1, 32, 32, 1280, 1280), (8, 128, 128, 320, 320),
              (8, 32, 32, 2560, 1280), (2, 16, 16, 320, 320), (1, 8, 8, 64, 72), (1, 64, 64, 960, 640)]
    for n, h, w, c, k in shapes:
        t8 = old(n, h, w, c, k, 3, 3, 1, 1)
        assert t8 in (90, 91, 92, 93)
        assert new(n, h, w, c, k, 3, 3, 1, 1, 0) == t8
        assert new(n, h, w, c, k, 3, 3, 1, 1, W4) == t8          # the W4 rule is the W8 rule ...
        assert new(n, h, w, c, k, 3, 3, 1, 1, W4 | 1 | (92 << 8)) == t8     # other bits are ignored
        assert new(n, h, w, c, k, 3, 3, 1, 1, W2) == 0
    assert old(1, 128, 128, 320, 320, 3, 3, 1, 1) == 92 and old(8, 128, 128, 320, 320, 3, 3, 1, 1) == 93
    # ... but for the measured exception: at most 16 output channels on the small patches (conv_out at batch 1)
    assert old(1, 128, 128, 320, 4, 3, 3, 1, 1) == 91 and new(1, 128, 128, 320, 4, 3, 3, 1, 1, W4) == 0
    assert old(8, 128, 128, 320, 4, 3, 3, 1, 1) == 92 and new(8, 128, 128, 320, 4, 3, 3, 1, 1, W4) == 92
    assert new(1, 128, 128, 320, 16, 3, 3, 1, 1, W4) == 0 and new(1, 128, 128, 320, 20, 3, 3, 1, 1, W4) == 91
    for flags in (0, W4):
        assert new(1, 12, 12, 960, 640, 3, 3, 1, 1, flags) == 0      # H % 8 != 0
        assert new(1, 16, 16, 320, 320, 3, 3, 2, 1, flags) == 0      # stride 2
        assert new(1, 16, 16, 320, 320, 1, 1, 1, 0, flags) == 0      # 1x1
        assert new(1, 16, 16, 48, 320, 3, 3, 1, 1, flags) == 0       # C % 64 != 0
        assert new(1, 16, 16, 96, 320, 3, 3, 1, 1, flags) == 0       # C % 32 == 0 is not enough


def test_halo_w4_switch_is_read_from_the_environment():
    """MIXDQ_HALO_W4=0 keeps packed convs on the implicit-GEMM family and leaves int8 convs alone."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    code = ("import ctypes; from mixdq_amd.build import build; lib = ctypes.CDLL(build()); "
            "f = lib.mixdq_conv_halo_select_flags; f.argtypes = [ctypes.c_int] * 10; "
            "print('IDS', f(1, 64, 64, 640, 640, 3, 3, 1, 1, 0), f(1, 64, 64, 640, 640, 3, 3, 1, 1, 2))")
    ids = {}
    for flag in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, MIXDQ_HALO_W4=flag),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:]
        ids[flag] = [int(v) for v in [ln for ln in r.stdout.splitlines() if ln.startswith("IDS ")][-1].split()[1:]]
    assert ids["1"][0] == ids["1"][1] == ids["0"][0] != 0
    assert ids["0"][1] == 0


class _StubLib:
    """Records what the Python layer asks the library."""

    def __init__(self, with_flags_query=True):
        self.calls = []
        if with_flags_query:
            self.mixdq_conv_halo_select_flags = self._flags

    def mixdq_conv_halo_select(self, *a):
        self.calls.append(("plain", a))
        return 90

    def _flags(self, *a):
        self.calls.append(("flags", a))
        return 92


def test_python_select_passes_the_w4_flag(monkeypatch):
    import mixdq_amd._C as C
    stub = _StubLib()
    monkeypatch.setattr(C, "_lib", stub)
    assert C.conv_halo_select(1, 64, 64, 640, 640, 3, 3, 1, 1) == 90
    assert C.conv_halo_select(1, 64, 64, 640, 640, 3, 3, 1, 1, w4=True) == 92
    assert stub.calls == [("plain", (1, 64, 64, 640, 640, 3, 3, 1, 1)),
                          ("flags", (1, 64, 64, 640, 640, 3, 3, 1, 1, C.FLAG_W4))]
    # the upsample fold asks about the conv's input size, twice the stored tensor's
    stub.calls.clear()
    assert C.conv_upsample2x_supported((2, 640, 32, 32), (640, 640, 3, 3), 1, 1, w4=True)
    assert stub.calls == [("flags", (2, 64, 64, 640, 640, 3, 3, 1, 1, C.FLAG_W4))]
    assert C.conv_upsample2x_supported((2, 640, 32, 32), (640, 640, 3, 3), 1, 1)
    assert stub.calls[-1][0] == "plain"
    # a library without the query has no W4 halo kernel
    monkeypatch.setattr(C, "_lib", _StubLib(with_flags_query=False))
    assert C.conv_halo_select(1, 64, 64, 640, 640, 3, 3, 1, 1, w4=True) == 0
    assert not C.conv_upsample2x_supported((2, 640, 32, 32), (640, 640, 3, 3), 1, 1, w4=True)


def test_module_asks_for_the_fold_with_its_own_storage(monkeypatch):
    """QuantizedConv2d.upsample2x_supported no longer excludes packed weights: it passes w4 on."""
    import mixdq_amd._C as C
    from mixdq_amd.nn.Conv2d import QuantizedConv2d
    seen = []
    monkeypatch.setattr(C, "conv_upsample2x_supported",
                        lambda x_shape, w_shape, stride, padding, w4=False: seen.append((w_shape, w4)) or True)

    class _M:
        valid_for_acceleration, split = True, 0
        out_channels, in_channels, kernel_size, stride, padding = 640, 640, (3, 3), (1, 1), (1, 1)
    for packed in (False, True):
        m = _M()
        m.w_packed4 = packed
        assert QuantizedConv2d.upsample2x_supported(m, (1, 640, 32, 32)) is True
    assert seen == [((640, 640, 3, 3), False), ((640, 640, 3, 3), True)]


class _Recorded(Exception):
    pass


@pytest.mark.parametrize("w4,cfg,want", [(True, 0, "conv_halo92"), (True, 93, "conv_halo93"), (False, 0, "conv_halo90"),
                                         (True, 4, "conv")])
def test_recorder_names_the_kernel_a_w4_launch_runs_on(monkeypatch, w4, cfg, want):
    """The launch recorder's `kind` (what the roofline pass of the benchmark turns into a kernel name): a W4
    launch that takes the halo kernel is `conv_halo{tile}`, as an int8 launch is."""
    import mixdq_amd._C as C
    monkeypatch.setattr(C, "_lib", _StubLib())
    monkeypatch.setattr(C, "_check", lambda cond, msg: None)        # (the is_cuda checks: no launch happens here)
    monkeypatch.setattr(C, "RECORD", [])

    def rec(kind, M, N, K, k_align, w4_, *rest, **kw):
        raise _Recorded(kind, (M, N, K, k_align), w4_)
    monkeypatch.setattr(C, "_record", rec)
    c, k = 128, 160
    x = torch.zeros(1, c, 16, 16, dtype=torch.int8).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(k, c // 2 if w4 else c, 3, 3, dtype=torch.int8)
    v = torch.ones(k)
    with pytest.raises(_Recorded) as e:
        C.qconv2d_w8_a8_ohalf(x, w, v, torch.tensor(1.0), torch.tensor(0.0), v, torch.ones(k, 1, 3, 3), None, None,
                              1, 1, _cfg=cfg, _w4=w4)
    assert e.value.args == (want, (256, k, 9 * c, c), w4)
