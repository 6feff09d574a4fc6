"""The strings that the decimal -> double converter of the device CSV parser (qe_csv_number.h) is checked on: by
tests/test_csv_device_cpu.py as host code, by tests/test_gpu_csv_device_scale.py as device code."""
import math
import struct


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def corpus(rng, scale=1):
    """`scale` multiplies the four random loop counts only: the fixed lists and the three 2000-step nextafter walks stay
    whole, so a smaller corpus keeps every edge."""
    out = []
    tiny, huge = 5e-324, 1.7976931348623157e308
    # repr of random doubles over the whole range (normal and subnormal), and the same values at 17 .. 25 digits
    for _ in range(int(150_000 * scale)):
        bits = rng.getrandbits(63)
        v = f64(bits)
        if math.isnan(v) or math.isinf(v):
            continue
        out.append(repr(v))
        out.append(f"{v:.{rng.randint(16, 24)}e}")
    # subnormals and the neighbourhood of DBL_MIN / DBL_MAX
    for _ in range(int(50_000 * scale)):
        v = f64(rng.getrandbits(52))
        out.append(repr(v))
        out.append(f"{v:.{rng.randint(16, 20)}e}")
    for base in (2.2250738585072014e-308, huge, tiny):
        v = base
        for _ in range(2000):
            out += [repr(v), f"{v:.17e}", f"{v:.18e}", f"{v:.20e}"]
            v = math.nextafter(v, 0.0)
    out += ["1.7976931348623158e308", "1.7976931348623159e308", "2.4703282292062327e-324", "2.4703282292062328e-324",
            "2.2250738585072011e-308", "2.2250738585072012e-308", "4.9406564584124654e-324", "1e-400", "1e309", "-1e-400"]
    # exact halfway points between neighbouring doubles (integers of <= 19 digits): round half to even
    for _ in range(int(100_000 * scale)):
        e = rng.randint(1, 11)
        m = rng.getrandbits(53) | (1 << 52)
        h = (2 * m + 1) << (e - 1)
        out.append(str(h))
        out.append(str(h + rng.choice((-1, 1))))
    # short decimals of every shape: what real files hold
    for _ in range(int(200_000 * scale)):
        ip = rng.randint(0, 10 ** rng.randint(0, 9))
        fp = rng.randint(0, 10 ** rng.randint(0, 8))
        s = f"{ip}.{fp}" if rng.random() < 0.8 else f"{ip}"
        if rng.random() < 0.2:
            s += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randint(0, 330))
        if rng.random() < 0.1:
            s = rng.choice("+-") + s
        if rng.random() < 0.05:
            s += rng.choice("dDfF")
        if rng.random() < 0.05:
            s = rng.choice([" ", "\t", " \x01"]) + s + rng.choice(["", " ", "\x0b"])
        out.append(s)
        out.append(f"{rng.uniform(0, 100):.2f}")
    out += [".5", "5.", "0.0", "-0", "-0.0e5", "+0", "00012.500", "0.000000000000000000000000001234", "1e0023", "1E-0",
            "NaN", "-NaN", "+NaN", "Infinity", "-Infinity", "+Infinity", " 2.5e1 ", "7d", "+1E2f", "7D", "1e400",
            "0x1p3", " 0x1.8p1 ", "0X.8P-1d", "-0x1.fffffffffffffp1023", "123456789012345678901234567890"]
    return out


def undecidable(s):
    """What the converter may leave to the host: a hexadecimal literal, or a decimal of more than 19 significant digits
    (leading zeros aside).  Everything else it has to decide itself."""
    body = s.strip("".join(chr(c) for c in range(0x21))).lstrip("+-")
    hexa = body[:2] in ("0x", "0X")
    digits = body.split("e")[0].split("E")[0].rstrip("dDfF").replace(".", "").lstrip("0")
    return hexa or len(digits) > 19
