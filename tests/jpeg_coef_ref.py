"""Baseline sequential JPEG entropy decoder (ITU-T T.81 annexes B, F.2 and figure A.6) in plain Python: the QUANTISED coefficients
a JPEG file carries, as an independent reading of what libjpeg wrote -- what jpeg2dct.loads hands the reference.  Test infrastructure
only; imports nothing of the product.

    comps = decode_coefficients(jpeg_bytes)
    comps[i].coef    int16 [blocks_y, blocks_x, 64]   natural (row-major u*8+v) order, NOT dequantised
    comps[i].qtable  int32 [64]                       natural order
    comps[i].h, .v   sampling factors

Handles DQT, SOF0, DHT and SOS, byte unstuffing, interleaved MCUs with sampling factors, single-component scans, DC prediction and the
zig-zag to natural order.  Refuses what it does not read: progressive / extended / arithmetic frames, restart intervals, 16-bit
tables, files with more than one scan per component."""
from collections import namedtuple

import numpy as np

Component = namedtuple("Component", "id h v coef qtable")

# T.81 figure A.6: ZIGZAG[k] = natural (row-major) position of the k-th coefficient in the scan
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
                   56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegError(ValueError):
    pass


def _huffman_table(counts, symbols):
    """T.81 annex C: canonical codes -> {(length, code): symbol}"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    """entropy-coded segment: 0xFF 0x00 is a stuffed 0xFF; any other marker ends the data"""

    def __init__(self, data, pos):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def _fill(self):
        d = self.data
        if self.pos >= len(d):
            raise JpegError("entropy-coded data ends early")
        b = d[self.pos]
        if b == 0xFF:
            nxt = d[self.pos + 1] if self.pos + 1 < len(d) else None
            if nxt != 0x00:
                raise JpegError("marker 0xFF%02X inside the entropy-coded data" % (nxt if nxt is not None else 0))
            self.pos += 2
        else:
            self.pos += 1
        self.acc = (self.acc << 8) | b
        self.n += 8

    def bit(self):
        if self.n == 0:
            self._fill()
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, count):
        v = 0
        for _ in range(count):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise JpegError("no Huffman code matches")

    def value(self, size):
        """T.81 F.2.2.1 EXTEND: `size` extra bits -> signed value"""
        if size == 0:
            return 0
        v = self.bits(size)
        return v if v >= (1 << (size - 1)) else v - (1 << size) + 1


def decode_coefficients(data):
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI marker")
    pos = 2
    qt, dc_tab, ac_tab = {}, {}, {}
    frame = None
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise JpegError("marker expected at byte %d" % pos)
        m = data[pos + 1]
        if m == 0xFF:                                    # fill byte
            pos += 1
            continue
        if m == 0xD9:
            raise JpegError("EOI before any scan")
        seg_len = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + seg_len]
        if len(seg) != seg_len - 2:
            raise JpegError("segment runs past the end of the file")
        pos += 2 + seg_len
        if m == 0xDB:                                    # DQT
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0:
                    raise JpegError("16-bit quantisation tables are not baseline")
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg[i + 1:i + 65], np.uint8)
                qt[tq] = t
                i += 65
        elif m == 0xC0:                                  # SOF0
            if frame is not None:
                raise JpegError("second frame header")
            if seg[0] != 8:
                raise JpegError("sample precision %d" % seg[0])
            height, width, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            frame = (height, width, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise JpegError("frame type 0xFF%02X (progressive / extended / lossless / arithmetic) is not baseline sequential" % m)
        elif m == 0xCC:
            raise JpegError("arithmetic coding conditioning")
        elif m == 0xC4:                                  # DHT
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                n = sum(counts)
                (ac_tab if tc else dc_tab)[th] = _huffman_table(counts, list(seg[i + 17:i + 17 + n]))
                i += 17 + n
        elif m == 0xDD:                                  # DRI
            if (seg[0] << 8) | seg[1]:
                raise JpegError("restart intervals are not supported")
        elif m == 0xDA:                                  # SOS
            break
        # APPn, COM and the rest carry no coefficients
    if frame is None:
        raise JpegError("scan before the frame header")
    height, width, comps = frame
    ns = seg[0]
    scan = [(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
    ss, se, ah_al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]
    if (ss, se, ah_al) != (0, 63, 0):
        raise JpegError("spectral selection / successive approximation in a baseline scan")
    if [c[0] for c in comps] != [s[0] for s in scan]:
        raise JpegError("one scan holding every component of the frame is what this decoder reads")
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if ns == 1:                                          # non-interleaved: one block per MCU, only the blocks that cover the component
        _, h, v, _ = comps[0]
        cw, chh = -(-width * h // hmax), -(-height * v // vmax)
        mcux, mcuy = -(-cw // 8), -(-chh // 8)
        per_mcu = [(1, 1)]
    else:
        mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
        per_mcu = [(c[1], c[2]) for c in comps]
    grids = [np.zeros((mcuy * v, mcux * h, 64), np.int16) for h, v in per_mcu]
    pred = [0] * len(comps)
    br = _Bits(data, pos)
    for my in range(mcuy):
        for mx in range(mcux):
            for ci, (h, v) in enumerate(per_mcu):
                dct, act = dc_tab[scan[ci][1]], ac_tab[scan[ci][2]]
                for by in range(v):
                    for bx in range(h):
                        blk = grids[ci][my * v + by, mx * h + bx]
                        pred[ci] += br.value(br.symbol(dct))
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = br.symbol(act)
                            run, size = rs >> 4, rs & 15
                            if size == 0:
                                if run == 15:            # ZRL: sixteen zeros
                                    k += 16
                                    continue
                                break                    # EOB
                            k += run
                            if k > 63:
                                raise JpegError("run past the end of a block")
                            blk[ZIGZAG[k]] = br.value(size)
                            k += 1
    if data[br.pos:br.pos + 2] != b"\xff\xd9":
        raise JpegError("no EOI after the scan (a second scan, or restart markers)")
    out = []
    for (cid, h, v, tq), g in zip(comps, grids):
        cw, chh = -(-width * h // hmax), -(-height * v // vmax)
        out.append(Component(cid, h, v, np.ascontiguousarray(g[:-(-chh // 8), :-(-cw // 8)]), qt[tq]))
    return out
