"""Lane-level host model of modinv_kernel<LPL> (csrc/mx_modinv.hpp) and of its dispatch in mx_modinv (csrc/mx_capi.hip).

Plain Python, no torch.  It is a CASE SELECTOR: it says which of the kernel's rare paths an operand pair reaches, so that the
directed tests can feed the device operands that reach them.  What is right is decided by pow(v, -1, m), never by this file.

A WaveInt<LPL> is 64 lanes x LPL 32-bit words, lane 0 least significant.  Here it is ONE Python int whose bits
[B*l, B*(l+1)), B = 32*LPL, are lane l — the same bits the kernel holds.  A "ballot" is an int with bit B*l set for lane l
(the kernel's 64-bit mask with its bits B apart), so that all 64 lanes are worked on by a handful of big-integer operations:

  sub_local / add_local   the lane-local chains of all lanes at once.  Even and odd lanes are handled apart, so that the
                          borrow / carry OUT of a lane lands in the empty slot above it and never enters the next lane:
                          exactly the kernel's b / c that stay in the lane until the ballots move them.
  ripple(G, P)            the kernel's  (P + (G << 1)) ^ P  with every lane widened from one bit to B bits: a propagating lane
                          is B one-bits, a carry that arrives at its bit 0 leaves at the top — the same addition.
  take_plus / take_minus  the lane's own +k / -k, wrapping inside the lane (the kernel's k ripple through the lane's words).

Every decision the kernel takes is taken here from the same quantities: the three-way branch on the low words, u_less from the
top lane's ballots (not from an integer comparison), equal from Z1, zeros() with its cap of 31, the bound 64 * limbs + 8,
m.gt(r) from the two ballots compared as integers, the word-wise and bit-wise halvings through add_mul with its carry word
handed to the next lane and the ripple of the add that follows.

modinv(v, m, limbs) returns (inverse or None, k, events).  EVENTS lists every name that can appear in `events`.
"""

from __future__ import annotations

from functools import lru_cache

LPLS = (1, 2, 3, 5, 9)
MAX_MOD_BITS = 29 * 9 * 64 - 4          # csrc/mx_host.hpp: the widest modulus any kernel of the library takes
WORD = 0xFFFFFFFF

EVENTS = (
    "add_propagate",          # r + s: a lane whose local sum is all ones receives a carry (the P ballot decides its carry out)
    "add_propagate_run2",     # ... in two or more consecutive lanes
    "sub_uv_propagate",       # u - v (taken): a lane whose local difference is zero receives a borrow
    "sub_uv_propagate_run2",
    "sub_vu_propagate",       # v - u (taken): the same
    "sub_vu_propagate_run2",
    "plus_k_ripple",          # take_plus: +k runs past word 0 of a lane (LPL > 1)
    "minus_k_ripple",         # take_minus: -k runs past word 0 of a lane (LPL > 1)
    "zero_low_word_u",        # zeros() sees a zero low word at the u shift (31 bits now, the rest next trip)
    "zero_low_word_v",        # ... at the v shift
    "zero_low_word_sub",      # ... after a subtraction
    "u_less_via_zero_top",    # u_less decided by Z1 >> 63 & cin1 >> 63 (top lane equal, borrow arrives)
    "equal_exit_u_is_one",    # v == u, u == 1: invertible
    "equal_exit_u_not_one",   # v == u, u != 1: gcd > 1
    "v_zero_on_entry",
    "r_ge_m",                 # !(m > r): the conditional subtraction is taken
    "r_lt_m",
    "tail_k_mod32_zero",
    "tail_k_mod32_nonzero",
    "add_mul_carry_ripple",   # add_mul: adding the lanes' carry words makes a carry cross a lane boundary
    "bound_reached",          # the loop ended by k >= bound with v != 0 (no input found that does)
)
IN_LANE_EVENTS = ("plus_k_ripple", "minus_k_ripple")     # do not exist for LPL = 1


class SizeError(ValueError):
    """mx_modinv returns MX_ERR_SIZE for this modulus / row width"""


def dispatch(bits: int, limbs: int):
    """the LPL instance mx_modinv launches for a modulus of `bits` bits in rows of `limbs` words; None: MX_ERR_SIZE"""
    if bits > MAX_MOD_BITS:
        return None
    need = max(limbs, (bits + 34 + 31) // 32)
    for lpl, cap in ((1, 64), (2, 128), (3, 192), (5, 320), (9, 576)):
        if need <= cap:
            return lpl
    return None


class Wave:
    """the constants of WaveInt<LPL> in the packed form"""

    def __init__(self, lpl: int):
        self.lpl = lpl
        B = self.B = 32 * lpl
        self.W = 64 * B
        self.MASK = (1 << self.W) - 1
        self.LANE = (1 << B) - 1
        self.ONES0 = sum(1 << (B * l) for l in range(64))                  # bit 0 of every lane: a ballot of all lanes
        self.EVEN = sum(self.LANE << (B * l) for l in range(0, 64, 2))
        self.ODD = self.EVEN << B
        self.OUT_E = sum(1 << (B * (l + 1)) for l in range(0, 64, 2))      # where the carry out of an even lane lands
        self.OUT_O = sum(1 << (B * (l + 1)) for l in range(1, 64, 2))      # ... of an odd lane (the top lane's: bit W)
        self.ONE_E = self.ONES0 & self.EVEN
        self.ONE_O = self.ONES0 & self.ODD
        self.LOW = self.ONES0 * WORD                                       # word 0 of every lane
        self.TOP = 1 << (B * 63)                                           # the top lane's ballot bit

    # ---- lane-local chains: (result words, ballot of the carry / borrow out of the lane, ballot "all ones" / "all zero")
    def _outs(self, xe: int, xo: int) -> int:
        return ((xe & self.OUT_E) | (xo & self.OUT_O)) >> self.B

    def sub_local(self, a: int, b: int):
        xe = ((a & self.EVEN) | self.OUT_E) - (b & self.EVEN)              # 2^B + a_l - b_l per lane: bit B clear = borrow
        xo = ((a & self.ODD) | self.OUT_O) - (b & self.ODD)
        w = (xe & self.EVEN) | (xo & self.ODD)
        borrow = self._outs(xe, xo) ^ self.ONES0
        nonzero = self._outs((w & self.EVEN) + self.EVEN, (w & self.ODD) + self.ODD)     # w_l + 2^B - 1 >= 2^B  <=>  w_l != 0
        return w, borrow, nonzero ^ self.ONES0

    def add_local(self, a: int, b: int):
        xe = (a & self.EVEN) + (b & self.EVEN)
        xo = (a & self.ODD) + (b & self.ODD)
        w = (xe & self.EVEN) | (xo & self.ODD)
        allones = self._outs((w & self.EVEN) + self.ONE_E, (w & self.ODD) + self.ONE_O)  # w_l + 1 = 2^B  <=>  all ones
        return w, self._outs(xe, xo), allones

    # ---- carries between lanes: the kernel's (P + (G << 1)) ^ P, the result truncated to the 64 lanes like its u64
    def ripple(self, G: int, P: int) -> int:
        pfull = P * self.LANE
        return ((pfull + (G << self.B)) ^ pfull) & self.ONES0

    def carry_in(self, G: int, P: int) -> int:
        """WaveInt::carry_in: the same formula, as add / sub / add_mul use it outside the main loop"""
        pfull = P * self.LANE
        return ((pfull + (G << self.B)) ^ pfull) & self.ONES0

    # ---- the lane's own +k / -k: k runs through the lane's words while they wrap, and stops at the lane's end
    def take_plus(self, w: int, cin: int, ev: set) -> int:
        if self.lpl > 1 and cin & self._word0_is(w, WORD):
            ev.add("plus_k_ripple")
        wrap = cin & self._outs((w & self.EVEN) + self.ONE_E, (w & self.ODD) + self.ONE_O)
        return (w + cin - (wrap << self.B)) & self.MASK

    def take_minus(self, w: int, cin: int, ev: set) -> int:
        if self.lpl > 1 and cin & self._word0_is(w, 0):
            ev.add("minus_k_ripple")
        nonzero = self._outs((w & self.EVEN) + self.EVEN, (w & self.ODD) + self.ODD)
        wrap = cin & (nonzero ^ self.ONES0)
        return (w - cin + (wrap << self.B)) & self.MASK

    def _word0_is(self, w: int, what: int) -> int:
        """ballot of the lanes whose word 0 is 0xFFFFFFFF (what = WORD) or 0 (what = 0); LPL > 1: bit 32 is inside the lane"""
        low = w & self.LOW
        if what:
            return ((low + self.ONES0) >> 32) & self.ONES0
        return (((low + self.LOW) >> 32) & self.ONES0) ^ self.ONES0

    # ---- WaveInt::add, ::sub, ::gt, ::add_mul
    def add(self, x: int, y: int, ev: set, tag=None) -> int:
        w, G, P = self.add_local(x, y)
        cin = self.carry_in(G, P)
        if tag and cin:
            ev.add(tag)
        return self.take_plus(w, cin, set())

    def sub(self, x: int, y: int) -> int:
        w, G, Z = self.sub_local(x, y)
        return self.take_minus(w, self.carry_in(G, Z), set())

    def gt(self, x: int, y: int) -> bool:
        _, borrow, zero = self.sub_local(x, y)
        return ((borrow | zero) ^ self.ONES0) > borrow                     # the two ballots compared as integers

    def add_mul(self, x: int, y: int, q: int, ev: set) -> int:
        xe = (x & self.EVEN) + q * (y & self.EVEN)                         # per lane x_l + q y_l < 2^(B+32): the carry WORD
        xo = (x & self.ODD) + q * (y & self.ODD)                           # lands in word 0 of the empty slot above
        low = (xe & self.EVEN) | (xo & self.ODD)
        carry_words = ((xe & self.ODD) | (xo & self.EVEN)) & self.MASK     # lane l <- lane l - 1; the top lane's is dropped
        return self.add(low, carry_words, ev, "add_mul_carry_ripple")


@lru_cache(maxsize=None)
def wave(lpl: int) -> Wave:
    return Wave(lpl)


def _zeros(low: int) -> int:
    return (low & -low).bit_length() - 1 if low else 31


def modinv(v: int, m: int, limbs=None, lpl=None):
    """(v^-1 mod m or None, k, events) as modinv_kernel computes them; SizeError where mx_modinv refuses the size.
    `limbs`: words per row (default: those of m); `lpl` overrides the dispatch."""
    if m < 3 or not m & 1:
        raise ValueError("modulus must be odd and >= 3")
    if limbs is None:
        limbs = max(1, (m.bit_length() + 31) // 32)
    if lpl is None:
        lpl = dispatch(m.bit_length(), limbs)
        if lpl is None:
            raise SizeError("modulus too large for the engine")
    wv = wave(lpl)
    B, ONES0, TOP = wv.B, wv.ONES0, wv.TOP
    ev: set = set()
    u, r, s, k = m, 0, 1, 0
    bound = 64 * limbs + 8
    vzero = v == 0
    if vzero:
        ev.add("v_zero_on_entry")
    while k < bound and not vzero:
        ul, vl = u & WORD, v & WORD
        if not ul & 1:
            n = _zeros(ul)
            if not ul:
                ev.add("zero_low_word_u")
            u >>= n
            s = (s << n) & wv.MASK
        elif not vl & 1:
            n = _zeros(vl)
            if not vl:
                ev.add("zero_low_word_v")
            v >>= n
            r = (r << n) & wv.MASK
        else:
            duv, G1, Z1 = wv.sub_local(u, v)
            dvu, G2, Z2 = wv.sub_local(v, u)
            sm, G3, P3 = wv.add_local(r, s)
            cin1, cin2, cin3 = wv.ripple(G1, Z1), wv.ripple(G2, Z2), wv.ripple(G3, P3)
            via_zero = bool(Z1 & cin1 & TOP)
            u_less = bool(G1 & TOP) or via_zero
            equal = not u_less and Z1 == ONES0
            if via_zero and not G1 & TOP:
                ev.add("u_less_via_zero_top")
            hit = P3 & cin3
            if hit:
                ev.add("add_propagate")
                if hit & (hit >> B):
                    ev.add("add_propagate_run2")
            if not u_less and not equal:
                hit = Z1 & cin1
                if hit:
                    ev.add("sub_uv_propagate")
                    if hit & (hit >> B):
                        ev.add("sub_uv_propagate_run2")
                u = wv.take_minus(duv, cin1, ev)
                r = wv.take_plus(sm, cin3, ev)
                n = _zeros(u & WORD)
                if not u & WORD:
                    ev.add("zero_low_word_sub")
                u >>= n
                s = (s << n) & wv.MASK
            else:
                hit = Z2 & cin2
                if hit:
                    ev.add("sub_vu_propagate")
                    if hit & (hit >> B):
                        ev.add("sub_vu_propagate_run2")
                v = wv.take_minus(dvu, cin2, ev)
                s = wv.take_plus(sm, cin3, ev)
                n = _zeros(v & WORD)
                if equal:
                    vzero, n = True, 1
                    ev.add("equal_exit_u_is_one" if u == 1 else "equal_exit_u_not_one")
                elif not v & WORD:
                    ev.add("zero_low_word_sub")
                v >>= n
                r = (r << n) & wv.MASK
        k += n
    if not vzero:
        ev.add("bound_reached")
    ok = vzero and u == 1
    if not wv.gt(m, r):
        ev.add("r_ge_m")
        r = wv.sub(r, m)
    else:
        ev.add("r_lt_m")
    x = wv.sub(m, r)
    minv = m & WORD
    for _ in range(4):
        minv = (minv * (2 - (m & WORD) * minv)) & WORD
    nminv = -minv & WORD
    left = k
    while left >= 32:
        x = wv.add_mul(x, m, ((x & WORD) * nminv) & WORD, ev) >> 32
        left -= 32
    ev.add("tail_k_mod32_nonzero" if left else "tail_k_mod32_zero")
    if left:
        x = wv.add_mul(x, m, ((x & WORD) * nminv) & WORD & ((1 << left) - 1), ev) >> left
    return (x & ((1 << (32 * limbs)) - 1) if ok else None), k, ev
