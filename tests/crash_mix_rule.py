"""Restatement, in Python, of which wavefronts of a mixed reuse sweep compute Stage A (csrc/qpn_internal.h, crash_mix_recomputes;
csrc/qpn_capi_nodes.hip, crash_mix_reuse_from and the two tuning constants).  The tests compare it with the C++ text and its
constants; nothing in the package imports it."""

RESIDENT = 16 * 256       # kResidentMI355X
SHARE = 96                # QPN_CRASH_MIX_SHARE: computing share of the mixed positions, in 1/256ths
TAIL = 0                  # QPN_CRASH_MIX_TAIL: reuse-only positions before the last partial round, in 1/256ths of RESIDENT
XCDS = 8


def reuse_from(batch, tail=None):
    tail = TAIL if tail is None else tail
    return max(0, (batch // RESIDENT) * RESIDENT - RESIDENT * tail // 256)


def phase(xcd):
    return 32 * (((xcd & 1) << 2) | (xcd & 2) | (xcd >> 2))


def recomputes(pos, share, from_):
    if pos >= from_:
        return False
    return ((((pos >> 3) * share + phase(pos & 7)) & 255) + share) >= 256


def mixed(batch, share=None):
    """Does a reuse sweep over `batch` resident nodes take the mixed instantiation?"""
    share = SHARE if share is None else share
    return share > 0 and batch > RESIDENT and reuse_from(batch) > 0
