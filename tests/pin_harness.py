"""What the pinning tests share: the measured-tolerance comparison and the guarded outputs.

A test module keeps its own table F (tensor kind -> factor, measured on the MI355X) and hands it to Checks; the bound is
    e_hip <= F[kind] * e_ref + FLOOR,     e_ref = max |oracle32 - oracle64| / max |oracle64|,  e_hip = max |hip - oracle64| / max |oracle64|
on the same inputs.  Outputs are views inside NaN-filled buffers with GUARD floats on each side: a store outside an output shows
in the bands, an element never written in the output, and what a call was told not to produce must still be NaN."""
import torch

FLOOR = 4 * 2.0 ** -23
GUARD = 256                          # floats on each side of an output (a multiple of 4: the view keeps the buffer's 16-byte alignment)
NAN = float("nan")


class Checks:
    """Prints e_ref, e_hip and their ratio for every compared tensor, then asserts all of them at once (one run shows every figure)."""

    def __init__(self, case, table):
        self.case, self.table, self.bad = case, table, []

    def add(self, kind, what, hip, o32, o64, denom=None, keep=None):
        F = self.table
        hip = hip.detach().cpu().double()
        assert hip.shape == o64.shape, (what, hip.shape, o64.shape)
        if keep is not None:
            keep = keep.expand_as(o64)
            hip, o32, o64 = hip[keep], o32[keep], o64[keep]
        assert bool(torch.isfinite(o64).all()) and o64.numel() > 0, "%s %s: the oracle itself" % (self.case, what)
        d = float(o64.abs().max()) if denom is None else float(denom)
        e_ref, e_hip = float((o32.double() - o64).abs().max()) / d, float((hip - o64).abs().max()) / d
        print("EDGE %-9s %-34s %-16s e_ref %.3e e_hip %.3e ratio %s need_F %.2f" % (
            kind, self.case, what, e_ref, e_hip, "%.2f" % (e_hip / e_ref) if e_ref > 0 else "-",
            max(e_hip - FLOOR, 0.0) / e_ref if e_ref > 0 else (0.0 if e_hip <= FLOOR else float("inf"))))
        if not e_hip <= F[kind] * e_ref + FLOOR:
            self.bad.append("%s %s: e_hip %.3e > %d * e_ref %.3e + %.1e" % (kind, what, e_hip, F[kind], e_ref, FLOOR))

    def done(self):
        assert not self.bad, "%s: %s" % (self.case, "; ".join(self.bad))


class Bufs:
    """The outputs of one launch: views inside NaN-filled buffers, GUARD floats on each side."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def new(self, name, *shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), NAN, device=self.dev)
        self.items.append((name, buf, n))
        return buf[GUARD:GUARD + n].view(*shape)

    def bands(self, what):
        for name, buf, n in self.items:
            ok = torch.stack([torch.isnan(buf[:GUARD]).all(), torch.isnan(buf[GUARD + n:]).all()]).tolist()
            assert ok[0] and ok[1], "%s: a store outside %s (guard band before: %s, after: %s)" % (what, name, ok[0], ok[1])


def written(v, what):
    assert bool(torch.isfinite(v).all()), "%s: non-finite values (an element never written, or poisoned)" % what


def untouched(v, what):
    assert bool(torch.isnan(v).all()), "%s: written, but the contract leaves it alone" % what
