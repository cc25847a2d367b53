"""TEST INFRASTRUCTURE (run as a child process by tests/test_inflate_hostile.py): gives every member of the file written by
`inflate_wave_check -c -w FILE` to pd_x_bgzf_inflate, one member per call, for the three kernels (variant 0, 1: one lane per
member, pd_inflate_core.h; 2: one wave per member, pd_inflate_wave.h), and compares with zlib.  Stops at the first failure, and at
the first error that is not a decoder's refusal (PD_X_BGZF_REFUSED: -(100 + |status|)): after a failed HIP call nothing more is launched.
What this leg can see on the device is a fault, a wrong verdict or wrong bytes inside [0, ISIZE): pd_x_bgzf_inflate allocates with plain
hipMalloc, not through the library's guarded allocations, so a stray device store that lands in mapped memory outside the output goes
unseen HERE.  That such stores do not happen is what the host run of the same source inside its fences shows; only members that passed
it are in the file."""
import sys
import zlib


def main(path, root):
    sys.path.insert(0, root)
    from pandepth_amd import capi
    data = open(path, "rb").read()
    rows = [ln.rstrip("\n").split("\t") for ln in open(path + ".tsv") if not ln.startswith("#")]
    n_ok = n_err = n_declined = 0
    for off, size, isize, zok, may_decline, wrong_crc, family, name in rows:
        off, size, isize, zok, may_decline, wrong_crc = int(off), int(size), int(isize), zok == "1", may_decline == "1", wrong_crc == "1"
        member = data[off:off + size]
        payload = member[18:-8]
        try:
            d = zlib.decompressobj(-15)
            ref = d.decompress(payload, isize + 1)
            ok = d.eof and len(ref) == isize
        except zlib.error:
            ok = False
        if ok != zok:
            print("FAIL %s: zlib here %s, zlib in the harness %s" % (name, ok, zok))
            return 1
        for variant in (0, 1, 2):
            try:
                out, _ms, _nb, n = capi.bgzf_inflate(member, variant=variant, reps=0)
                err = None
            except capi.PdError as e:
                out, err = None, e
                if not -199 <= e.code <= -101:
                    print("FAIL %s: variant %d: %s is not a decoder's refusal: stopping" % (name, variant, e))
                    return 1
                if wrong_crc and ok and variant == 2 and e.code != -120:
                    print("FAIL %s: variant %d: refused with %d, not for the CRC-32 (-120)" % (name, variant, e.code))
                    return 1
            # (the lane-per-member kernels do not look at the CRC-32; the wave kernel does)
            must_fail = not ok or (wrong_crc and variant == 2)
            may_fail = must_fail or (variant == 2 and may_decline)
            if err is None and must_fail:
                print("FAIL %s: variant %d accepted it (zlib: %s, wrong CRC: %s)" % (name, variant, ok, wrong_crc))
                return 1
            if err is not None and not may_fail:
                print("FAIL %s: variant %d: %s on a member zlib inflates" % (name, variant, err))
                return 1
            if err is None and out != ref:
                print("FAIL %s: variant %d: bytes differ from zlib's" % (name, variant))
                return 1
            n_ok += err is None
            n_err += err is not None
            n_declined += err is not None and ok and not wrong_crc
    print("hostile members: %d members x 3 kernels: %d inflated to zlib's bytes, %d refused (%d of them declined by the wave kernel), 0 failures" % (len(rows), n_ok, n_err, n_declined))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
