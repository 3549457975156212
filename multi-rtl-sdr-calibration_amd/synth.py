"""Seeded synthetic 8x-oversampled GSM BCCH-carrier IQ (uint8, interleaved I,Q) and the GMSK
modulator that also produces the SCH training-sequence template.

Nothing here is derived from reference code: the reference gets its template from MathWorks'
comm.GMSKModulator (gsm_SCH_training_sequence_gen.m:14,39 -- Communications Toolbox, not in the
repo) and its IQ from RTL-SDR dongles.  What is taken from the reference is data: the 64 SCH
extended-training bits (gsm_SCH_training_sequence_gen.m:17-19), the differential pre-coding rule
d = ~xor(b[i], b[i-1]) with b[-1] = 0 (:32), BT = 0.3, pulse length 4, 8 samples/symbol (:9-14),
and the burst geometry SCH_corr_rate_correction.m:22-27 assumes (training sequence 42 symbols
into the SCH burst, SCH one frame after FCCH).

Stream model: 51-multiframe on slot 0 -- FCCH at frames 0,10,20,30,40, SCH one
frame later, BCCH at frames 2..5, normal bursts elsewhere, idle frame 50 -- slots 1..7 carry
random normal bursts at equal power; per-stream sampling-clock error (resampling), carrier
error, AWGN, DC offset, uint8 quantisation.  RNG: numpy Philox keyed by (seed, dongle, arfcn).
"""
from __future__ import annotations

import math

import numpy as np

SYMBOL_RATE = (1625.0 / 6.0) * 1e3
OV = 8
FS = SYMBOL_RATE * OV
FRAME_OV = 1250 * OV  # 10 000 samples per TDMA frame at 8x
SLOT_OV = 1250        # 156.25 symbols * 8
BURST_BITS = 148

SCH_TRAINING_BITS = np.array(
    [1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0,
     0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 0, 0,
     1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1], dtype=np.int8)

# GSM 05.02 normal-burst training sequence code 0 (26 bits)
TSC0 = np.array([0, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 1, 1], dtype=np.int8)

# GSM 05.02 table 5.2.3a: the eight normal-burst training sequence codes (the bits gsm_normal_training_sequence_gen.m:18-25
# lists); TSC[k] is what a cell with base-station colour code k sends in every normal burst of its BCCH carrier
TSC = np.array([
    [0, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 1, 1],
    [0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1],
    [0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0],
    [0, 1, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 0],
    [0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1],
    [0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0],
    [1, 0, 1, 0, 0, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 1],
    [1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0]], dtype=np.int8)

DEFAULT_SEED = 20260101

# ---- the SCH payload (GSM 05.03 section 4.7, 04.08 section 9.1.30): BSIC and reduced frame number ---------------------------
HYPERFRAME = 2048 * 26 * 51                      # 2 715 648 TDMA frames
# the bit map, one row per information bit d(0..24): (field, bit of that field).  T1 = FN div 1326 (11 bits), T2 = FN mod 26,
# T3P = (FN mod 51 - 1) / 10.  Unpinned against a real capture: this table is the one place to pin it.
SCH_INFO_MAP = (
    ("T1", 9), ("T1", 10), ("BSIC", 0), ("BSIC", 1), ("BSIC", 2), ("BSIC", 3), ("BSIC", 4), ("BSIC", 5),
    ("T1", 1), ("T1", 2), ("T1", 3), ("T1", 4), ("T1", 5), ("T1", 6), ("T1", 7), ("T1", 8),
    ("T3P", 1), ("T3P", 2), ("T2", 0), ("T2", 1), ("T2", 2), ("T2", 3), ("T2", 4), ("T1", 0), ("T3P", 0))
SCH_CRC_POLY = 0b10101110101                     # g(D) = D^10 + D^8 + D^6 + D^5 + D^4 + D^2 + 1
SCH_CODED_FIRST, SCH_CODED_SECOND = 3, 106       # burst bits 3..41 carry c(0..38), 106..144 carry c(39..77)


def sch_info_bits(bsic, fn):
    """The 25 information bits d(0..24) of the SCH burst of TDMA frame fn (fn mod 51 in 1, 11, 21, 31, 41)."""
    bsic, fn = int(bsic), int(fn)
    t3 = fn % 51
    if not (0 <= bsic < 64 and 0 <= fn < HYPERFRAME and t3 % 10 == 1 and t3 < 50):
        raise ValueError("sch_info_bits: bsic 0..63, fn an SCH frame of the hyperframe")
    val = {"BSIC": bsic, "T1": fn // 1326, "T2": fn % 26, "T3P": (t3 - 1) // 10}
    return np.array([(val[f] >> b) & 1 for f, b in SCH_INFO_MAP], dtype=np.int8)


def sch_fields(d):
    """d(0..24) -> dict(bsic, t1, t2, t3p, fn); fn = 1326 T1 + 51 ((T3 - T2) mod 26) + T3 with T3 = 10 T3' + 1."""
    val = {"BSIC": 0, "T1": 0, "T2": 0, "T3P": 0}
    for bit, (f, b) in zip(np.asarray(d).tolist(), SCH_INFO_MAP):
        val[f] |= int(bit) << b
    t3 = 10 * val["T3P"] + 1
    return {"bsic": val["BSIC"], "t1": val["T1"], "t2": val["T2"], "t3p": val["T3P"],
            "fn": 1326 * val["T1"] + 51 * ((t3 - val["T2"]) % 26) + t3}


def sch_crc_remainder(word):
    """remainder (10 bits, as an integer, D^9 the top bit) of the bit sequence `word` (first bit = highest power) divided by g(D)"""
    reg = 0
    for bit in np.asarray(word).tolist():
        reg = (reg << 1) | int(bit)
        if reg & 0x400:
            reg ^= SCH_CRC_POLY
    return reg


def sch_conv_encode(u):
    """rate 1/2: c(2k) = u(k)+u(k-3)+u(k-4), c(2k+1) = u(k)+u(k-1)+u(k-3)+u(k-4), u(k<0) = 0"""
    u = np.asarray(u, dtype=np.int8)
    z = np.concatenate([np.zeros(4, np.int8), u])
    c = np.empty(2 * len(u), dtype=np.int8)
    c[0::2] = z[4:] ^ z[1:-3] ^ z[:-4]
    c[1::2] = z[4:] ^ z[3:-1] ^ z[1:-3] ^ z[:-4]
    return c


def sch_encode(bsic, fn):
    """The 78 coded bits c(0..77) of the SCH burst of frame fn: 25 information bits, 10 parity bits (the inverted remainder, so
    that the 35-bit word leaves all ones), 4 zero tail bits, the rate-1/2 code.  No interleaving."""
    d = sch_info_bits(bsic, fn)
    rem = sch_crc_remainder(np.concatenate([d, np.zeros(10, np.int8)])) ^ 0x3FF
    par = np.array([(rem >> (9 - i)) & 1 for i in range(10)], dtype=np.int8)
    return sch_conv_encode(np.concatenate([d, par, np.zeros(4, np.int8)]))


def sch_plant(bits, bsic, fn):
    """overwrite the 78 payload bits of the 148 SCH burst bits (in place)"""
    c = sch_encode(bsic, fn)
    bits[SCH_CODED_FIRST:SCH_CODED_FIRST + 39] = c[:39]
    bits[SCH_CODED_SECOND:SCH_CODED_SECOND + 39] = c[39:]
    return bits


# ---- the BCCH block (GSM 05.03 section 4.1: SACCH / BCCH coding): 23 octets of system information over four normal bursts ----
FIRE_POLY = sum(1 << k for k in (40, 26, 23, 17, 3, 0))    # g(D) = (D^23 + 1)(D^17 + D^3 + 1)
FIRE_ONES = (1 << 40) - 1
BCCH_FRAMES = (2, 3, 4, 5)                       # frames of the 51-multiframe whose slot 0 carries the BCCH block
SI_MESSAGE_TYPE = {1: 0x19, 2: 0x1A, 3: 0x1B, 4: 0x1C}     # 04.08 section 10.4
SI_FILL = 0x2B


def bcch_bit_order(octets):
    """23 octets -> d(0..183), d(8n + k) = bit k of octet n (LSB first).  Unpinned against a real capture: this
    function and bcch_octets below are the one place to pin the order."""
    o = np.asarray(octets, dtype=np.int64).ravel()
    if o.shape != (23,) or np.any(o < 0) or np.any(o > 255):
        raise ValueError("a BCCH block is 23 octets")
    return ((o[:, None] >> np.arange(8)[None, :]) & 1).astype(np.int8).ravel()


def bcch_octets(d):
    """the inverse of bcch_bit_order: d(0..183) -> (23,) uint8"""
    d = np.asarray(d, dtype=np.int64).reshape(23, 8)
    return np.sum(d << np.arange(8)[None, :], axis=1).astype(np.uint8)


def fire_remainder(word):
    """remainder (40 bits, as an integer, D^39 the top bit) of the bit sequence `word` (first bit = highest power) divided by the
    Fire code's g(D) = D^40 + D^26 + D^23 + D^17 + D^3 + 1"""
    reg = 0
    for bit in np.asarray(word).tolist():
        reg = (reg << 1) | int(bit)
        if reg >> 40:
            reg ^= FIRE_POLY
    return reg


def bcch_interleave_map():
    """(456, 2): coded bit c(k) goes to burst B = k mod 4 of the block, position j = 2 ((49 k) mod 57) + ((k mod 8) div 4) of that
    burst's 114 data bits"""
    k = np.arange(456)
    return np.stack([k % 4, 2 * ((49 * k) % 57) + (k % 8) // 4], axis=1)


def bcch_data_symbol(j):
    """data bit i(B, j), j = 0..113 -> its bit of the 148-bit normal burst: e(j) for j < 57, e(j + 2) behind the two stealing
    flags e(57), e(58); e(0..57) are burst bits 3..60 and e(58..115) burst bits 87..144"""
    j = np.asarray(j)
    return np.where(j < 57, 3 + j, 31 + j)


BCCH_STEAL_SYMBOLS = (60, 87)                    # e(57), e(58)


def bcch_block_encode(octets):
    """23 octets -> (4, 116) int8, the e(B, 0..115) of the block's four bursts: 184 information bits, 40 parity bits (the inverted
    Fire remainder, so that the 224-bit word leaves all ones), 4 zero tail bits, the rate-1/2 code of the SCH (the same generators),
    the interleaver of 05.03 section 4.1.4, and the two stealing flags set."""
    d = bcch_bit_order(octets)
    rem = fire_remainder(np.concatenate([d, np.zeros(40, np.int8)])) ^ FIRE_ONES
    par = np.array([(rem >> (39 - i)) & 1 for i in range(40)], dtype=np.int8)
    c = sch_conv_encode(np.concatenate([d, par, np.zeros(4, np.int8)]))
    m = bcch_interleave_map()
    i = np.zeros((4, 114), dtype=np.int8)
    i[m[:, 0], m[:, 1]] = c
    e = np.ones((4, 116), dtype=np.int8)
    e[:, :57] = i[:, :57]
    e[:, 59:] = i[:, 57:]
    return e


def bcch_plant(bits, e):
    """overwrite the 116 payload bits (stealing flags included) of the 148 normal-burst bits (in place)"""
    bits[3:61] = e[:58]
    bits[87:145] = e[58:]
    return bits


def _bcd_digits(value, what, allowed):
    s = value if isinstance(value, str) else ("%d" % int(value)).rjust(min(allowed), "0")
    if not s.isdigit() or len(s) not in allowed:
        raise ValueError("%s: %s decimal digits" % (what, " or ".join(str(a) for a in allowed)))
    return [int(ch) for ch in s]


def lai_octets(mcc, mnc, lac):
    """The five octets of the location area identification (04.08 section 10.5.1.3): MCC digit 2 | digit 1, MNC digit 3 | MCC
    digit 3, MNC digit 2 | digit 1, then the LAC big-endian.  mnc: an int below 100 is a 2-digit MNC (its third digit is the
    filler 0xF), 100..999 a 3-digit one; a string gives the digits as written ("012")."""
    m, n = _bcd_digits(mcc, "mcc", (3,)), _bcd_digits(mnc, "mnc", (2, 3))
    lac = int(lac)
    if not 0 <= lac <= 0xFFFF:
        raise ValueError("lac: 0..65535")
    n3 = n[2] if len(n) == 3 else 0xF
    return [m[1] << 4 | m[0], n3 << 4 | m[2], n[1] << 4 | n[0], lac >> 8, lac & 0xFF]


def _si_octets(si_type, length, body):
    o = [(length << 2) | 1, 0x06, SI_MESSAGE_TYPE[si_type]] + body
    return np.array(o + [SI_FILL] * (23 - len(o)), dtype=np.uint8)


def si3_octets(cell_id, mcc, mnc, lac):
    """A SYSTEM INFORMATION TYPE 3 block: L2 pseudo-length, protocol discriminator 0x06, message type 0x1B, the cell identity
    in octets 3-4 (big-endian), the LAI in octets 5-9, the rest 0x2B"""
    cell_id = int(cell_id)
    if not 0 <= cell_id <= 0xFFFF:
        raise ValueError("cell_id: 0..65535")
    return _si_octets(3, 18, [cell_id >> 8, cell_id & 0xFF] + lai_octets(mcc, mnc, lac))


def si4_octets(mcc, mnc, lac):
    """A SYSTEM INFORMATION TYPE 4 block: the LAI in octets 3-7"""
    return _si_octets(4, 12, lai_octets(mcc, mnc, lac))


def si_fields(octets):
    """The Python statement of gsmcal_si_fields (include/gsmcal_si.h): 23 octets -> dict(valid, msg_type, si_type, cell_id, mcc,
    mnc, mnc_digits, lac); the fields are -1 where the message does not carry them, valid is 0 for anything not recognised
    (another pseudo-length form or protocol discriminator, another message type, BCD digits above 9 other than the MNC filler)."""
    o = [int(v) for v in np.asarray(octets).ravel()]
    out = {"valid": 0, "msg_type": o[2], "si_type": 0, "cell_id": -1, "mcc": -1, "mnc": -1, "mnc_digits": -1, "lac": -1}
    if len(o) != 23 or (o[0] & 3) != 1 or o[1] != 0x06:
        return out
    types = {v: k for k, v in SI_MESSAGE_TYPE.items()}
    if o[2] not in types:
        return out
    out["si_type"] = types[o[2]]
    if out["si_type"] < 3:
        out["valid"] = 1
        return out
    at = 5 if out["si_type"] == 3 else 3
    m = [o[at] & 15, o[at] >> 4, o[at + 1] & 15]
    n = [o[at + 2] & 15, o[at + 2] >> 4, o[at + 1] >> 4]
    if max(m) > 9 or max(n[:2]) > 9 or (n[2] > 9 and n[2] != 0xF):
        return out
    if out["si_type"] == 3:
        out["cell_id"] = o[3] << 8 | o[4]
    out["mcc"] = 100 * m[0] + 10 * m[1] + m[2]
    out["mnc_digits"] = 2 if n[2] == 0xF else 3
    out["mnc"] = 10 * n[0] + n[1] if n[2] == 0xF else 100 * n[0] + 10 * n[1] + n[2]
    out["lac"] = o[at + 3] << 8 | o[at + 4]
    out["valid"] = 1
    return out


def _si_args(si):
    """si= of ideal_waveform / make_stream -> a (count, 23) uint8 array, or None"""
    if si is None:
        return None
    a = np.asarray(si)
    a = a.reshape(1, 23) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[1] != 23 or a.shape[0] < 1 or np.any(a < 0) or np.any(a > 255):
        raise ValueError("si: 23 octets, or a sequence of such blocks")
    return a.astype(np.uint8)


def _qfunc(x):
    return 0.5 * np.array([math.erfc(v / math.sqrt(2.0)) for v in np.ravel(x)]).reshape(np.shape(x))


def gmsk_frequency_pulse(bt=0.3, pulse_len=4, sps=OV):
    """Gaussian-filtered rectangular frequency pulse g[n], truncated to pulse_len symbols, sampled
    at sample centres, normalised so that sum(g) = 1/2 (one symbol moves the phase by pi/2)."""
    n = pulse_len * sps
    t = (np.arange(n) + 0.5) / sps - pulse_len / 2.0  # in symbol periods
    k = 2.0 * math.pi * bt / math.sqrt(math.log(2.0))
    g = _qfunc(k * (t - 0.5)) - _qfunc(k * (t + 0.5))
    return g * (0.5 / np.sum(g))


_G = gmsk_frequency_pulse()


def diff_precode(bits, prev=0):
    """d[i] = NOT(b[i] xor b[i-1]), b[-1] = prev (gsm_SCH_training_sequence_gen.m:32)."""
    b = np.concatenate([[prev], np.asarray(bits, dtype=np.int8)])
    return (1 - np.abs(np.diff(b))).astype(np.int8)


def gmsk_modulate(precoded_bits, sps=OV, g=None):
    """Unit-modulus GMSK of pre-coded bits (0 -> -1, 1 -> +1), phase starts at 0, output length
    len(bits)*sps (the pulse's own delay of pulse_len/2 symbols is inside the output, as with a
    streaming modulator)."""
    g = _G if g is None else g
    a = 2.0 * np.asarray(precoded_bits, dtype=np.float64) - 1.0
    up = np.zeros(len(a) * sps)
    up[::sps] = a
    f = np.convolve(up, g)[: len(up)]
    phase = math.pi * np.cumsum(f)
    return np.exp(1j * phase)


def sch_training_sequence(sps=OV):
    """512 x 1 complex template: stand-in for gsm_SCH_training_sequence_gen(8)."""
    return gmsk_modulate(diff_precode(SCH_TRAINING_BITS), sps)


def normal_training_sequences(sps=OV):
    """(26*sps, 8) complex templates, column k = TSC[k] modulated: stand-in for gsm_normal_training_sequence_gen(sps)."""
    g = gmsk_frequency_pulse(sps=sps)
    return np.stack([gmsk_modulate(diff_precode(TSC[k]), sps, g) for k in range(8)], axis=1)


def fir1(n, wn):
    """Own statement of fir1(n, Wn) (low-pass, Hamming window, unit DC gain), as used at
    gsm_sync_demod.m:34 / multi_rtl_sdr_gsm_FCCH_scanner.m:53."""
    k = np.arange(n + 1, dtype=np.float64)
    m = k - n / 2.0
    h = wn * np.sinc(wn * m)
    w = 0.54 - 0.46 * np.cos(2.0 * math.pi * k / n)
    h = h * w
    # MATLAB builds both the ideal response and the window as one half plus its mirror image, so the taps it
    # returns are symmetric to the last bit; do the same (the HIP front end has a faster kernel for such taps)
    half = (n + 1) // 2
    h[n + 1 - half:] = h[:half][::-1]
    return h / np.sum(h)


def _burst_bits(kind, rng, tsc=0):
    if kind == "F":
        return np.zeros(BURST_BITS, dtype=np.int8)
    if kind == "S":
        return np.concatenate([np.zeros(3, np.int8), rng.integers(0, 2, 39, dtype=np.int8),
                               SCH_TRAINING_BITS, rng.integers(0, 2, 39, dtype=np.int8),
                               np.zeros(3, np.int8)])
    # normal burst: 3 tail, 58 data(+stealing), 26 TSC, 58 data, 3 tail
    return np.concatenate([np.zeros(3, np.int8), rng.integers(0, 2, 58, dtype=np.int8), TSC[tsc],
                           rng.integers(0, 2, 58, dtype=np.int8), np.zeros(3, np.int8)])


def _slot0_kind(frame_in_mf):
    f = frame_in_mf % 51
    if f == 50:
        return "I"
    if f % 10 == 0:
        return "F"
    if f % 10 == 1:
        return "S"
    return "N"


def _ramp(n_total, n_edge=8):
    w = np.ones(n_total)
    e = 0.5 - 0.5 * np.cos(math.pi * (np.arange(n_edge) + 0.5) / n_edge)
    w[:n_edge] = e
    w[-n_edge:] = e[::-1]
    return w


_RAMP = _ramp(BURST_BITS * OV)


def _sch_payload_args(start_frame, bsic, fn0):
    """(bsic, fn0) to plant, or None: either argument switches the planted payload on, the other then takes its default"""
    if bsic is None and fn0 is None:
        return None
    bsic, fn0 = (0 if bsic is None else int(bsic)), (int(start_frame) if fn0 is None else int(fn0))
    if not 0 <= bsic < 64 or not 0 <= fn0 < HYPERFRAME or fn0 % 51 != start_frame:
        raise ValueError("bsic must be 0..63 and fn0 a frame of the hyperframe with fn0 mod 51 == start_frame")
    return bsic, fn0


def ideal_waveform(num_frames, start_frame, rng, bcch=True, tsc=0, bsic=None, fn0=None, si=None):
    """Complex baseband at exactly 8 samples/symbol, num_frames TDMA frames starting at frame
    `start_frame` of the 51-multiframe.  bcch=False gives a traffic-only carrier (no FCCH/SCH).
    tsc: the training sequence code (0..7) every normal burst carries.
    bsic / fn0: plant sch_encode(bsic, fn0 + frame) in every SCH burst (fn0 mod 51 == start_frame; the frame number wraps at
    HYPERFRAME).  The random payload is drawn first and then overwritten, so everything else of the waveform is unchanged.
    si: 23 octets, or a sequence of such blocks: bcch_block_encode(si[(frame number div 51) mod len(si)]) is planted in the slot-0
    bursts of frames 2..5 of every multiframe (the frame number counts from fn0, or from start_frame without one), again over
    the random payload that was drawn first."""
    payload = _sch_payload_args(start_frame, bsic, fn0)
    blocks = _si_args(si) if bcch else None
    coded = {}
    n = num_frames * FRAME_OV
    x = np.zeros(n, dtype=np.complex128)
    # all bursts of the stream are modulated in one vectorised pass: bits -> (nb, 148)
    kinds = []
    for fr in range(num_frames):
        k0 = _slot0_kind(start_frame + fr) if bcch else "N"
        kinds.append(k0)
        kinds.extend(["N"] * 7)
    nb = len(kinds)
    # every burst is modulated with PRE guard bits in front and POST behind (zeros, like the tail
    # bits) so that the phase trajectory is already established at the burst's first sample; the
    # burst-local sample 0 is the instant bit 0's frequency pulse starts -- the same convention as
    # gmsk_modulate()/sch_training_sequence(), so the SCH training sequence sits 42*8 samples in.
    PRE, POST = 4, 4
    nbits = PRE + BURST_BITS + POST
    bits = np.zeros((nb, nbits), dtype=np.int8)
    for i, k in enumerate(kinds):
        bits[i, PRE:PRE + BURST_BITS] = _burst_bits("N" if k == "I" else k, rng, tsc)
        if k == "S" and payload is not None:
            sch_plant(bits[i, PRE:PRE + BURST_BITS], payload[0], (payload[1] + i // 8) % HYPERFRAME)
        if blocks is not None and i % 8 == 0 and (start_frame + i // 8) % 51 in BCCH_FRAMES:
            fn = ((start_frame if payload is None else payload[1]) + i // 8) % HYPERFRAME
            which = (fn // 51) % len(blocks)
            if which not in coded:
                coded[which] = bcch_block_encode(blocks[which])
            bcch_plant(bits[i, PRE:PRE + BURST_BITS], coded[which][(start_frame + i // 8) % 51 - BCCH_FRAMES[0]])
    prev = np.concatenate([np.zeros((nb, 1), np.int8), bits[:, :-1]], axis=1)
    pre = 1 - np.abs(bits - prev)                       # diff_precode per burst
    a = 2.0 * pre.astype(np.float64) - 1.0
    up = np.zeros((nb, nbits * OV))
    up[:, ::OV] = a
    # causal convolution with g along time, truncated to the burst length
    f = np.zeros_like(up)
    for j, gj in enumerate(_G):
        f[:, j:] += gj * up[:, : up.shape[1] - j]
    ph = math.pi * np.cumsum(f, axis=1) + rng.uniform(0, 2 * math.pi, (nb, 1))
    b = np.exp(1j * ph[:, PRE * OV: (PRE + BURST_BITS) * OV]) * _RAMP[None, :]
    for i, k in enumerate(kinds):
        if k == "I":
            continue
        fr, sl = divmod(i, 8)
        s0 = fr * FRAME_OV + sl * SLOT_OV
        x[s0: s0 + BURST_BITS * OV] = b[i]
    return x


def _iq_impair(y, iq_gain, iq_phase_deg):
    """The front end's I/Q imbalance on a complex waveform: I = x_I, Q = g*(x_Q cos(phi) + x_I sin(phi)) (either argument left at
    None: g = 1 / phi = 0)."""
    g = 1.0 if iq_gain is None else float(iq_gain)
    phi = 0.0 if iq_phase_deg is None else math.radians(float(iq_phase_deg))
    return y.real + 1j * (g * (y.imag * math.cos(phi) + y.real * math.sin(phi)))


def make_stream(dongle=0, arfcn=0, num_frames=102, seed=DEFAULT_SEED, bcch=True,
                sampling_ppm=None, carrier_ppm=None, snr_db=None, carrier_freq=957.4e6,
                start_frame=None, frac_start=None, tx_key=None, tsc=0, bsic=None, fn0=None, si=None,
                iq_gain=None, iq_phase_deg=None):
    """One capture: returns (raw uint8 interleaved I,Q of length 2*num_frames*10000, truth dict).
    tx_key: dongles given the same key receive the SAME transmission (payload, multiframe phase, start instant) through
    their own clocks, carrier offsets and noise -- what gsm_sync_demod.m's inter-dongle phase plot (:151-158) looks at.
    With tx_key, a start_frame or frac_start left at None is drawn from the transmission's generator BEFORE the payload: two
    dongles share the payload only when both leave the argument at None or both give it (pair_coherence needs the same payload).
    tsc: the cell's training sequence code (0..7), planted in every normal burst.
    bsic / fn0: the SCH payload (ideal_waveform): the cell's BSIC and the GSM frame number of the waveform's first frame, which
    needs start_frame given with fn0 mod 51 == start_frame.  Left at None the SCH payload stays random and the capture is
    byte-identical to what it always was.
    si: the system information the BCCH blocks carry (ideal_waveform; si3_octets / si4_octets build one); None leaves their
    payload random and the capture byte-identical likewise.
    iq_gain / iq_phase_deg: the front end's gain ratio g and quadrature skew phi (_iq_impair), applied to the noisy waveform before
    the DC and the rounding; with both left at None nothing is applied and the capture is byte-identical likewise."""
    rng = np.random.Generator(np.random.Philox(key=[int(seed), (int(dongle) << 20) ^ int(arfcn)]))
    eps_s = rng.uniform(-80.0, 80.0) if sampling_ppm is None else float(sampling_ppm)
    eps_c = rng.uniform(-40.0, 40.0) if carrier_ppm is None else float(carrier_ppm)
    snr = rng.uniform(15.0, 30.0) if snr_db is None else float(snr_db)
    sf = int(rng.integers(0, 51)) if start_frame is None else int(start_frame)
    fs0 = rng.uniform(0.0, FRAME_OV) if frac_start is None else float(frac_start)
    n = num_frames * FRAME_OV
    if tx_key is None:
        ideal = ideal_waveform(num_frames + 2, sf, rng, bcch=bcch, tsc=tsc, bsic=bsic, fn0=fn0, si=si)
    else:
        txr = np.random.Generator(np.random.Philox(key=[int(seed) ^ 0x5A5A5A5A, int(tx_key)]))
        if start_frame is None:
            sf = int(txr.integers(0, 51))
        if frac_start is None:
            fs0 = txr.uniform(0.0, FRAME_OV)
        ideal = ideal_waveform(num_frames + 2, sf, txr, bcch=bcch, tsc=tsc, bsic=bsic, fn0=fn0, si=si)
    # the dongle's clock runs (1+eps_s) fast => sample k is taken at ideal time k/(1+eps_s)... the
    # estimator's sign convention (FCCH_fine_correction.m:111-115): observed spacing = ideal*(1+e)
    # means the dongle takes MORE samples per GSM frame, i.e. query ideal time t_k = k/(1+e).
    e = eps_s * 1e-6
    t = fs0 + np.arange(n, dtype=np.float64) / (1.0 + e)
    i0 = np.floor(t).astype(np.int64)
    fr = t - i0
    # 4-point cubic (Catmull-Rom) interpolation of the 8x-oversampled waveform
    xm1, x0, x1, x2 = ideal[i0 - 1 + 1], ideal[i0 + 1], ideal[i0 + 2], ideal[i0 + 3]
    y = x0 + 0.5 * fr * (x1 - xm1 + fr * (2 * xm1 - 5 * x0 + 4 * x1 - x2 + fr * (3 * (x0 - x1) + x2 - xm1)))
    f_off = eps_c * 1e-6 * carrier_freq
    y = y * np.exp(1j * (2.0 * math.pi * f_off / FS * np.arange(n) + rng.uniform(0, 2 * math.pi)))
    amp = 70.0
    sigma = amp * 10.0 ** (-snr / 20.0) / math.sqrt(2.0)
    y = amp * y + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if iq_gain is not None or iq_phase_deg is not None:
        y = _iq_impair(y, iq_gain, iq_phase_deg)
    dc = 127.4 + rng.uniform(-1.0, 1.0, 2)
    raw = np.empty(2 * n, dtype=np.float64)
    raw[0::2] = y.real + dc[0]
    raw[1::2] = y.imag + dc[1]
    raw = np.clip(np.floor(raw + 0.5), 0, 255).astype(np.uint8)
    truth = {"sampling_ppm": eps_s, "carrier_ppm": eps_c, "snr_db": snr, "start_frame": sf,
             "frac_start": fs0, "carrier_freq": carrier_freq, "bcch": bcch}
    payload = _sch_payload_args(sf, bsic, fn0) if bcch else None
    truth["bsic"], truth["fn0"] = payload if payload is not None else (None, None)
    truth["si"] = _si_args(si) if bcch else None
    truth["iq_gain"], truth["iq_phase_deg"] = iq_gain, iq_phase_deg
    return raw, truth


def make_cw(n, step=0.7, amp=100.0, dc=(127.4, 127.6), noise=0.5, drops=(), seed=DEFAULT_SEED, iq_gain=None, iq_phase_deg=None):
    """A CW capture as check_CW_samples_loss_tcp.m records one from a signal generator: the tone amp*exp(1i*(step*t + phi)) plus
    white Gaussian noise (standard deviation `noise` per component) plus DC, rounded and clipped to bytes; returns the 2n
    interleaved uint8 I,Q bytes.  drops = [(pos, k), ...] removes k samples of the source after output index pos (0-based), so
    CW_check's spike of k*step (mod 2 pi) lands at n = pos + 1 (1-based).  iq_gain / iq_phase_deg: the front end's I/Q imbalance
    (_iq_impair) on the noisy tone before the DC and the rounding; both None: nothing is applied, the bytes are what they always were."""
    rng = np.random.Generator(np.random.Philox(key=[int(seed), 0x4357 ^ int(n)]))
    gap = np.zeros(n, dtype=np.int64)
    for pos, k in drops:
        if not 0 <= pos < n - 1:
            raise ValueError("a drop must lie between two output samples")
        gap[pos + 1] += int(k)
    t = np.arange(n, dtype=np.float64) + np.cumsum(gap)
    y = amp * np.exp(1j * (step * t + rng.uniform(0, 2 * math.pi)))
    y = y + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if iq_gain is not None or iq_phase_deg is not None:
        y = _iq_impair(y, iq_gain, iq_phase_deg)
    raw = np.empty(2 * n, dtype=np.float64)
    raw[0::2] = y.real + dc[0]
    raw[1::2] = y.imag + dc[1]
    return np.clip(np.floor(raw + 0.5), 0, 255).astype(np.uint8)


def make_wideband(dongle=0, n=100000, sample_rate=2.048e6, tuned_freq=433.92e6, e_ppm=0.0, c_ppm=0.0, start=0.0, phase=0.0, tx_key=0,
                  tones=96, band=0.3, amp=30.0, dc=(127.4, 127.6), noise=0.5, iq_gain=None, iq_phase_deg=None, seed=DEFAULT_SEED):
    """One capture of a wide-band transmission at any centre frequency and sample rate, as a retuned dongle records it: returns (raw
    uint8 interleaved I,Q of length 2n, truth dict).  The transmission of (seed, tx_key) is a sum of `tones` unit tones over sqrt(tones)
    (unit power), their frequencies uniform in +-band/2 cycles per nominal sample, their phases uniform: s(t) = sum_i exp(j (2 pi nu_i t
    + theta_i)) / sqrt(tones), t in nominal sample periods.  It is evaluated EXACTLY at the dongle's sample times -- there is no
    interpolator in the generator, so what a resampler leaves is the resampler's.  make_stream's convention: dongle sample k is taken
    at nominal time (start + k) / (1 + e), e = 1e-6 e_ppm, and turned by 2 pi f_off k / sample_rate + phase, f_off = 1e-6 c_ppm
    tuned_freq.  Then amp, white Gaussian noise (standard deviation `noise` per component, from the generator of (seed, dongle)), the
    I/Q imbalance (_iq_impair; both None: none), DC, rounding and clipping to bytes as in make_cw."""
    txr = np.random.Generator(np.random.Philox(key=[int(seed) ^ 0x57494445, int(tx_key)]))
    nu = txr.uniform(-0.5 * band, 0.5 * band, int(tones))
    theta = txr.uniform(0.0, 2.0 * math.pi, int(tones))
    rng = np.random.Generator(np.random.Philox(key=[int(seed), 0x5742 ^ (int(dongle) << 20)]))
    e = 1e-6 * float(e_ppm)
    f_off = 1e-6 * float(c_ppm) * float(tuned_freq)
    y = np.empty(n, dtype=np.complex128)
    for lo in range(0, n, 1 << 16):                                   # (the (chunk, tones) phase matrix stays small)
        k = np.arange(lo, min(lo + (1 << 16), n), dtype=np.float64)
        t = (float(start) + k) / (1.0 + e)
        s_t = np.exp(1j * (2.0 * math.pi * np.outer(t, nu) + theta)).sum(axis=1) / math.sqrt(int(tones))
        y[lo: lo + len(k)] = s_t * np.exp(1j * (2.0 * math.pi * f_off / float(sample_rate) * k + float(phase)))
    y = float(amp) * y + float(noise) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if iq_gain is not None or iq_phase_deg is not None:
        y = _iq_impair(y, iq_gain, iq_phase_deg)
    raw = np.empty(2 * n, dtype=np.float64)
    raw[0::2] = y.real + dc[0]
    raw[1::2] = y.imag + dc[1]
    raw = np.clip(np.floor(raw + 0.5), 0, 255).astype(np.uint8)
    truth = {"e_ppm": float(e_ppm), "c_ppm": float(c_ppm), "f_off": f_off, "start": float(start), "phase": float(phase),
             "sample_rate": float(sample_rate), "tuned_freq": float(tuned_freq), "tx_key": int(tx_key), "nu": nu, "theta": theta}
    return raw, truth


# ------------------------------------------------------------------------------------------------
# Host twin of the device-side capture expansion (csrc/kernels_frontend.h: k_synth_expand).
# ------------------------------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(x):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return x ^ (x >> np.uint64(31))


def expand_capture(base, unit, seed=DEFAULT_SEED):
    """Capture `unit` of gsmcal_synth_expand_dev(base, ...): base is (K, 2N) uint8.  Bit-identical to the device kernel."""
    base = np.asarray(base, dtype=np.uint8)
    k, two_n = base.shape
    n = two_n // 2
    with np.errstate(over="ignore"):
        u = np.uint64(unit)
        sh = int(_mix64(np.uint64(seed) ^ (u * np.uint64(0xD1B54A32D192ED03))) % np.uint64(n))
        key = _mix64(np.uint64(seed) + np.uint64(0x632BE59BD9B4E019) * u)
    b = base[int(unit) % k].reshape(n, 2)
    src = (np.arange(n, dtype=np.int64) + sh) % n
    z = _mix64(key ^ np.arange(n, dtype=np.uint64))
    di = (z & np.uint64(3)).astype(np.int64)
    dq = ((z >> np.uint64(2)) & np.uint64(3)).astype(np.int64)
    out = np.empty((n, 2), dtype=np.int64)
    out[:, 0] = b[src, 0].astype(np.int64) + (di == 0) - (di == 1)
    out[:, 1] = b[src, 1].astype(np.int64) + (dq == 0) - (dq == 1)
    return np.clip(out, 0, 255).astype(np.uint8).reshape(-1)
