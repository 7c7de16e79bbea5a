"""A seeded corpus for the host-side scan reader (csrc/meshio.hip: tgn_obj_count / tgn_obj_read / tgn_vertex_normals /
tgn_scan_open / tgn_scan_take): OBJ texts from a small grammar plus byte-level mutation, ground-truth JSON documents from
json.dumps plus mutation, meshes for the vertex normals, and whole scans.  Pure Python, no GPU, no product import: the
differential test (tests/test_scan_reader_fuzz.py) and the sanitized stand-alone harness (tests/host/, fed by
`python tests/scan_reader_cases.py --dump DIR`) read the same cases.  Every case is a function of (kind, seed) alone.
"""
import json
import os
import random
import re
import struct
import sys

# How hard the mutated sets are hit: each of MAX_MUTATIONS slots of a case applies one mutation with this probability.  The test
# asserts that under the ORACLE alone each mutated set both parses and raises in at least 30 % of its cases (a condition on the
# inputs, not a tolerance).  Measured with the seeds below at 0.06: OBJ 892 of 1400 parse (63.7 %) and 508 raise (36.3 %); JSON 527 of
# 1400 parse (37.6 %) and 873 raise (62.4 %).  At 0.0 the oracle raises on 13 % of the OBJ set and on none of the JSON set, at 1.0 it
# parses 16 % and 0.1 %: either end fails the share assertion.
MUTATION_RATE = 0.06
MAX_MUTATIONS = 24

OBJ_GRAMMAR_SEEDS = range(400)
OBJ_MUTATED_SEEDS = range(1400)
JSON_VALID_SEEDS = range(300)
JSON_MUTATED_SEEDS = range(1400)
MESH_SEEDS = range(300)

ALPHABET = [b"_", b"(", b")", b"/", b"+", b"-", b".", b"e", b"x", b"\0", b"\t", b"\v", b"\f", b"\x1c", b"\x85", b"\xa0",
            "\u00a0".encode(), "\u2003".encode(), "\uff11".encode(), b"\xff",
            b" ", b"\n", b"\r", b"0", b"1", b"7", b"9", b"v", b"f", b"n", b"a", b"i", b"E"]
JSON_ALPHABET = ALPHABET + [b"[", b"]", b"{", b"}", b'"', b"\\", b",", b":", b"t", b"u"]
STRETCH = (59, 60, 61, 64, 399, 400, 401, 408)          # the edges of the parsers' two stack buffers (char[64], char[408])


def _rng(kind, seed):
    return random.Random(f"{kind}:{seed}")              # a str seed is hashed with sha512: the same stream in every process


# ---- OBJ ---------------------------------------------------------------------------------------------------------------------
def _cased(rng, word):
    return "".join(c.upper() if rng.random() < 0.5 else c.lower() for c in word)


def _coordinate(rng):
    k = rng.randrange(14)
    if k < 4:
        return "%.6f" % rng.uniform(-40, 40)
    if k == 4:
        return str(rng.randrange(-50, 50))
    if k == 5:
        return rng.choice("+-") + "%.3f" % rng.uniform(0, 9)
    if k == 6:
        return "%s%de%s%d" % (rng.choice(["", "-", "+"]), rng.randrange(1, 99), rng.choice(["", "+", "-"]), rng.randrange(0, 30))
    if k == 7:
        return "%.4fE%d" % (rng.uniform(-9, 9), rng.randrange(-12, 12))
    if k == 8:
        return rng.choice([".5", "5.", "-.25", "+7.", "-.5e+2", "0.", ".0", "00012.50"])
    if k == 9:
        return rng.choice(["", "-", "+"]) + _cased(rng, rng.choice(["inf", "nan", "infinity"]))
    if k == 10:
        return rng.choice(["4.9e-324", "2.2250738585072014e-308", "1e-310", "-3e-320", "2.4703282292062328e-324"])   # subnormals
    if k == 11:
        return rng.choice(["1e400", "-1e999", "1e-400", "-1e-999", "17976931348623157e292", "1.7976931348623159e308"])
    if k == 12:
        return rng.choice(["0.1000000000000000055511151231257827", "123456789.123456789e-5", "9007199254740993", "0.30000000000000004"])
    return "%.17g" % rng.uniform(-1e3, 1e3)


def _sep(rng):
    return rng.choice([" ", " ", " ", "\t", "  ", " \t", "\v", "\f "])


def _obj_lines(rng):
    lines, nv = [], 0
    style = rng.choice(["plain", "plain", "slashes", "mixed"])
    for _ in range(rng.randrange(0, 14)):
        k = rng.randrange(10)
        lead = rng.choice(["", "", "", " ", "\t"])
        if k < 4:
            toks = ["v"] + [_coordinate(rng) for _ in range(3)]
            if rng.random() < 0.25:
                toks += [_coordinate(rng) for _ in range(rng.randrange(1, 4))]      # colours behind the coordinates: ignored
            nv += 1
        elif k < 7:
            ref = [rng.randrange(1, max(nv, 1) + 1) for _ in range(3)]
            how = style if style != "mixed" else rng.choice(["plain", "slashes", "full"])
            if rng.random() < 0.03:
                how = "full"
            if how == "plain":
                toks = ["f"] + [str(r) for r in ref]
            elif how == "slashes":
                toks = ["f"] + ["%d//%d" % (r, rng.randrange(1, 9)) for r in ref]
            else:
                toks = ["f"] + ["%d/%d/%d" % (r, r, r) for r in ref]                  # int("1/1/1") raises
            if rng.random() < 0.2:
                toks.append(str(rng.randrange(1, 9)))                                 # a quad's fourth corner: ignored
        else:
            toks = rng.choice([["vn", "0", "0", "1"], ["vt", "0.5", "0.5"], ["#", "v", "1", "2", "x"], ["#comment"], ["g", "scan"],
                               ["vp", "1", "2"], ["vv", "1", "2", "3"], ["o", "name"], ["s", "off"], ["fv", "1", "2", "3"],
                               ["usemtl", "m_1"], ["vertex", "1", "2", "3"]])
        lines.append(lead + _sep(rng).join(toks) + rng.choice(["", "", " ", "\t"]))
    if lines and rng.random() < 0.2:                                                  # a blank line in the middle ends the read
        lines.insert(rng.randrange(len(lines) + 1), rng.choice(["", " ", " \t ", "\t"]))
    return lines


def obj_grammar(seed):
    """An unmutated OBJ text (bytes)."""
    rng = _rng("obj", seed)
    if seed % 50 == 0:
        return b""
    if seed % 50 == 1:
        return rng.choice([b"v", b"f", b"\n", b"\r", b" ", b"#", b"1", b"\0"])
    lines = _obj_lines(rng)
    ends = rng.choice([["\n"], ["\n"], ["\r\n"], ["\r"], ["\n", "\r\n", "\r"]])
    text = "".join(line + rng.choice(ends) for line in lines)
    if text and rng.random() < 0.3:
        text = text.rstrip("\r\n")                                                     # the last line without a terminator
    return text.encode()


def _stretch(rng, data):
    """pads one token that holds a digit with zeros in front of its first digit until the token is STRETCH characters long"""
    toks = [m for m in re.finditer(rb"[^\s\x1c-\x1f]*[0-9][^\s\x1c-\x1f]*", data)]
    if not toks:
        return data
    m = rng.choice(toks)
    want = rng.choice(STRETCH)
    at = m.start() + re.search(rb"[0-9]", m.group()).start()
    return data[:at] + b"0" * max(want - len(m.group()), 0) + data[at:]


def _mutate_once(rng, data, alphabet, extra=()):
    ops = ["delete", "insert", "insert", "replace", "replace", "truncate", "dupline", "stretch", "payload"] + list(extra)
    op = rng.choice(ops)
    n = len(data)
    at = rng.randrange(n + 1)
    if op == "delete" and n:
        at = min(at, n - 1)
        return data[:at] + data[at + 1:]
    if op == "insert":
        return data[:at] + rng.choice(alphabet) + data[at:]
    if op == "replace" and n:
        at = min(at, n - 1)
        return data[:at] + rng.choice(alphabet) + data[at + 1:]
    if op == "truncate" and "truncated" not in extra:
        return data[:at]
    if op == "dupline":
        lines = data.splitlines(keepends=True)
        if lines:
            i = rng.randrange(len(lines))
            lines.insert(i, lines[i])
            return b"".join(lines)
    if op == "stretch":
        return _stretch(rng, data)
    if op == "payload":                                                                # "nan(123)": C's strtod takes it, float() does not
        nans = [m.end() for m in re.finditer(rb"(?i)nan", data)]
        if nans:
            i = rng.choice(nans)
            return data[:i] + b"(" + rng.choice([b"", b"1", b"abc", b"0x7"]) + b")" + data[i:]
    if op == "swap":                                                                   # [ <-> {, ] <-> }
        where = [i for i, c in enumerate(data) if c in b"[]{}"]
        if where:
            i = rng.choice(where)
            return data[:i] + bytes([b"{}[]"[b"[]{}".index(data[i])]]) + data[i + 1:]
    if op == "bom":
        return b"\xef\xbb\xbf" + data
    if op == "control":                                                                # a raw control character inside a string
        where = [m.start() + 1 for m in re.finditer(rb'"[^"\\]', data)]
        if where:
            i = rng.choice(where)
            return data[:i] + bytes([rng.choice([0, 1, 9, 10, 13, 27, 31])]) + data[i:]
    if op == "backslash":                                                              # a backslash as the last byte
        return data[:at] + b"\\"
    if op in ("digits", "zeros"):
        nums = [m for m in re.finditer(rb"(?<=[\[ ,\n\t])-?[0-9]+(?=[\], \n\t,])", data)]
        if nums:
            m = rng.choice(nums)
            new = (rng.choice([b"", b"-"]) + rng.choice([b"1", b"9"]) * rng.choice([17, 18, 19])) if op == "digits" else \
                rng.choice([b"-0", b"01", b"-01", b"00"])
            return data[:m.start()] + new + data[m.end():]
    return data


def _mutate(rng, data, alphabet, extra=()):
    for _ in range(MAX_MUTATIONS):
        if rng.random() < MUTATION_RATE:
            data, before = _mutate_once(rng, data, alphabet, extra), data
            if len(data) < len(before) - 1:
                extra = tuple(extra) + ("truncated",)        # a file is cut short once, not over and over until nothing is left
    return data


def obj_mutated(seed):
    rng = _rng("obj-mut", seed)
    return _mutate(rng, obj_grammar(rng.randrange(2, 10 ** 6) * 50 + rng.randrange(2, 50)), ALPHABET)


# The divergences the differential was written after (tests/test_scan_reader_fuzz.py holds each by name).
NAMED_OBJ = {
    "mac_line_ends": b"v 1 2 3\rv 4 5 6\rf 1 2 1\r",
    "double_cr_blank_line": b"v 1 2 3\r\rv 4 5 6\n",
    "nan_payload": b"v nan(abc) 2 3\n",
    "underscore_in_float": b"v 1_0 2 3\n",
    "underscore_in_int": b"v 1 2 3\nf 1_0 2 3\n",
    "nbsp_is_white_space": b"v 1 2 3" + "\u00a0".encode() + b"4\n",
    "x1c_is_white_space": b"v 1 2 3\x1cv 4 5 6\n",
    "coordinate_over_400_chars": b"v " + b"0" * 420 + b"1.5 2 3\n",
    "face_index_over_60_chars": b"v 1 2 3\nf " + b"0" * 70 + b"1 1 1\n",
}
NAMED_JSON = {
    "garbage_inside_a_container": b'{"x": [tru, @@], "jaw": "upper", "labels": [1]}',
    "object_without_colon": b'{"x": {"a" 1}, "jaw": "upper", "labels": [1]}',
    "raw_tab_in_a_key": b'{"jaw": "upper", "k\tk": 1, "labels": [1]}',
}


# ---- ground-truth JSON -------------------------------------------------------------------------------------------------------
def _json_string(rng):
    parts = ["tooth", "AB12", ']}"', '"', "\\", "\n", "\t", "/", "\u00e9", "\u2003", "\U0001f9b7", "\x7f", "labels", "jaw", " ", "\b\f\r"]
    return "".join(rng.choice(parts) for _ in range(rng.randrange(0, 5)))


def _json_value(rng, depth=0):
    k = rng.randrange(11 if depth < 3 else 8)
    if k == 0:
        return rng.randrange(-100, 100)
    if k == 1:
        return rng.choice([0.5, -1.5e-3, 1e300, 2.5e-308, 123456.789, -0.0, 1e22])
    if k == 2:
        return rng.choice([True, False, None])
    if k == 3:
        return rng.choice([float("nan"), float("inf"), float("-inf")])
    if k < 7:
        return _json_string(rng)
    if k == 7:
        return [rng.randrange(0, 17) for _ in range(rng.randrange(0, 6))]
    if k < 10:
        return [_json_value(rng, depth + 1) for _ in range(rng.randrange(0, 4))]
    return {_json_string(rng): _json_value(rng, depth + 1) for _ in range(rng.randrange(0, 4))}


def json_valid(seed):
    """-> (document bytes, the labels json.load yields, the jaw): valid JSON with plain-int "labels" and a plain-ASCII "jaw"."""
    rng = _rng("json", seed)
    labels = [rng.randrange(-3, 61) for _ in range(rng.randrange(0, 13))]
    jaw = rng.choice(["upper", "lower", "upper", "lower", "Lower", ""])
    members = []
    if rng.random() < 0.5:
        members.append(("id_patient", rng.choice(["AB12", "0EJBIPTC", _json_string(rng)])))
    if rng.random() < 0.5:
        members.append(("instances", [rng.randrange(0, 9) for _ in labels]))
    for _ in range(rng.randrange(0, 4)):
        members.append((rng.choice(["x", "meta", "labels2", "Jaw", "k k", "\u00fcber", _json_string(rng)]), _json_value(rng)))
    members = [(k, v) for k, v in dict(members).items() if k not in ("jaw", "labels")] + [("jaw", jaw), ("labels", labels)]
    rng.shuffle(members)
    doc = dict(members)
    indent = rng.choice([None, None, 0, 1, 2, "\t"])
    separators = rng.choice([None, (",", ":"), (" , ", " : "), (",\n", ":\r\n")])
    text = json.dumps(doc, indent=indent, separators=separators, ensure_ascii=rng.random() < 0.5)
    how = rng.randrange(8)
    if how == 0:                                           # a duplicate "labels" key written by hand: the LAST one counts
        text = '{"labels": [9, 9, 9], ' + text[1:].lstrip()
    elif how == 1:
        labels = [rng.randrange(0, 49) for _ in labels]
        text = text.rstrip()[:-1].rstrip() + ', "labels": %s}' % json.dumps(labels)
    if rng.random() < 0.3:
        text = rng.choice([" ", "\n", "\r\n\t"]) + text + rng.choice(["\n", " \r\n", "\t"])
    return text.encode("utf-8"), labels, jaw


def json_mutated(seed):
    """-> (document bytes, the number of labels of the document it was mutated from)"""
    rng = _rng("json-mut", seed)
    text, labels, _ = json_valid(rng.randrange(10 ** 6))
    return _mutate(rng, text, JSON_ALPHABET, extra=("swap", "bom", "control", "backslash", "digits", "zeros")), len(labels)


def plain_obj(n, faces=True):
    """a well-formed OBJ of n vertices (bytes), the partner of a JSON case with n labels"""
    lines = ["v %d.5 %d %d.25" % (i, (i * 7) % 5, -i) for i in range(n)]
    if faces and n >= 3:
        lines += ["f %d %d %d" % (i + 1, i + 2, i + 3) for i in range(n - 2)]
    return ("\n".join(lines) + ("\n" if lines else "")).encode()


# ---- meshes for the vertex normals -------------------------------------------------------------------------------------------
def mesh(seed):
    """-> (vertices: list of [x, y, z], triangles: list of [a, b, c] zero-based); some hold an index of -1 or nv on purpose."""
    rng = _rng("mesh", seed)
    nv = rng.choice([0, 1, 2, 3, 4, 5, 8, 12])
    scale = rng.choice([1.0, 1.0, 1.0, 1e150, 1e-150, 1e160, 1e-170, 5e-324])
    special = rng.choice([[], [], [], [float("inf")], [float("nan")], [float("-inf"), float("nan")], [0.0, -0.0]])

    def coordinate():
        if special and rng.random() < 0.15:
            return rng.choice(special)
        return rng.choice([rng.uniform(-3, 3), float(rng.randrange(-3, 4))]) * scale

    vertices = [[coordinate(), coordinate(), coordinate()] for _ in range(nv)]
    if nv >= 3 and rng.random() < 0.3:                      # three collinear points
        vertices[1] = [2 * a for a in vertices[0]]
        vertices[2] = [3 * a for a in vertices[0]]
    triangles = []
    if nv:
        used = rng.randrange(1, nv + 1)                     # vertices behind `used` stay unreferenced
        for _ in range(rng.choice([0, 1, 2, 5, 20])):
            t = [rng.randrange(used) for _ in range(3)]
            if rng.random() < 0.2:
                t[1] = t[0]                                 # degenerate: a == b
            triangles.append(t)
            if rng.random() < 0.2:
                triangles.append(list(t))                   # repeated
    bad = seed % 10
    if bad == 0:
        triangles.insert(rng.randrange(len(triangles) + 1), [0, -1, 0] if nv else [-1, -1, -1])
    elif bad == 1:
        triangles.insert(rng.randrange(len(triangles) + 1), [0, nv, 0] if nv else [0, 0, 0])
    return vertices, triangles


# ---- whole scans -------------------------------------------------------------------------------------------------------------
def scans():
    """-> [(name, obj bytes, json bytes)]: 0 / 1 / 2 / 24 000 / 24 001 vertices, the jaw strings, labels across -3 .. 60, a label count
    off by one in each direction."""
    out = []
    every = list(range(-3, 61))
    for n in (0, 1, 2, 24000, 24001):
        for jaw in (("upper", "lower", "Lower", "") if n <= 2 else ("lower",) if n == 24000 else ("upper",)):
            labels = [every[(i * 37 + n) % len(every)] for i in range(n)]
            out.append((f"n{n}_{jaw or 'empty'}", plain_obj(n), json.dumps({"jaw": jaw, "labels": labels}).encode()))
    for n in (0, 1, 2, 64):
        for jaw in ("upper", "lower"):
            for off in (-1, 1):
                if n + off >= 0:
                    labels = [every[(i * 11) % len(every)] for i in range(n + off)]
                    out.append((f"n{n}_{jaw}_labels{off:+d}", plain_obj(n), json.dumps({"labels": labels, "jaw": jaw}).encode()))
    out.append(("all_labels_upper", plain_obj(64), json.dumps({"jaw": "upper", "labels": every}).encode()))
    out.append(("all_labels_lower", plain_obj(64), json.dumps({"jaw": "lower", "labels": every}, indent=1).encode()))
    return out


# ---- the dump the stand-alone harness reads ----------------------------------------------------------------------------------
def dump(directory):
    """NAME.obj + NAME.json pairs (tgn_obj_count / tgn_obj_read / tgn_vertex_normals on the OBJ, tgn_scan_open / tgn_scan_take on the
    pair) and NAME.mesh files (int64 nv, int64 nf, nv*3 doubles, nf*3 int64, little endian: tgn_vertex_normals).  Returns the counts."""
    os.makedirs(directory, exist_ok=True)
    pairs = []
    some_json = b'{"jaw": "lower", "labels": [31, 32, 48]}'
    for s in OBJ_GRAMMAR_SEEDS:
        pairs.append((f"obj_grammar_{s}", obj_grammar(s), some_json))
    for s in OBJ_MUTATED_SEEDS:
        pairs.append((f"obj_mutated_{s}", obj_mutated(s), some_json))
    for name, text in NAMED_OBJ.items():
        pairs.append((f"obj_named_{name}", text, some_json))
    for s in JSON_VALID_SEEDS:
        text, labels, _ = json_valid(s)
        pairs.append((f"json_valid_{s}", plain_obj(len(labels)), text))
    for s in JSON_MUTATED_SEEDS:
        text, n = json_mutated(s)
        pairs.append((f"json_mutated_{s}", plain_obj(n), text))
    for name, text in NAMED_JSON.items():
        pairs.append((f"json_named_{name}", plain_obj(1), text))
    pairs += [(f"scan_{name}", o, j) for name, o, j in scans()]
    for name, o, j in pairs:
        with open(os.path.join(directory, name + ".obj"), "wb") as st:
            st.write(o)
        with open(os.path.join(directory, name + ".json"), "wb") as st:
            st.write(j)
    for s in MESH_SEEDS:
        v, t = mesh(s)
        with open(os.path.join(directory, f"mesh_{s}.mesh"), "wb") as st:
            st.write(struct.pack("<qq", len(v), len(t)))
            st.write(struct.pack("<%dd" % (len(v) * 3), *[x for row in v for x in row]))
            st.write(struct.pack("<%dq" % (len(t) * 3), *[x for row in t for x in row]))
    return len(pairs), len(MESH_SEEDS)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--dump":
        sys.exit("usage: python tests/scan_reader_cases.py --dump DIR")
    n_pairs, n_meshes = dump(sys.argv[2])
    print(f"{n_pairs} OBJ + JSON pairs and {n_meshes} meshes written to {sys.argv[2]}")
