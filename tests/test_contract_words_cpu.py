"""The words every kernel has to agree on are stated once: the bits of the status word (include/ddz_env.h, mirrored in
engine.py), the domains of the RNG (csrc/ddz_device.h), the meta row of a fresh deal.  Read from the sources; no GPU, no
build."""
import glob
import importlib
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "doudizhu-rl_amd", "csrc")

STATUS = ["MISMATCH", "CAPACITY", "BAD_LAST", "AUTO_WAIT", "AUTO_DEPTH", "Q_NO_ROW", "DOMAIN", "CFR_CAPACITY", "SOLVE_DEPTH"]
RNG = ["DEAL", "STEP", "EPSILON", "PLAYOUT", "WORLD", "EXPAND", "TREE_PLAYOUT", "CFR_CHOOSE"]


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(files) >= 18
    return {os.path.basename(f): open(f).read() for f in files}


def call_text(text, start):
    """the text of the call whose opening parenthesis is the first one at or after `start`, up to the matching one"""
    i = text.index("(", start)
    depth = 0
    for j in range(i, len(text)):
        depth += (text[j] == "(") - (text[j] == ")")
        if depth == 0:
            return text[i:j + 1]
    raise AssertionError("unbalanced call")


def test_status_bits_named_once():
    hdr = open(os.path.join(REPO, "include", "ddz_env.h")).read()
    enum = re.findall(r"^\s*DDZ_ST_([A-Z_]+) = (\d+),?$", hdr, re.M)
    assert [n for n, _ in enum] == STATUS
    assert [int(v) for _, v in enum] == [1 << k for k in range(9)]
    engine = importlib.import_module("doudizhu-rl_amd.engine")
    pkg = importlib.import_module("doudizhu-rl_amd")
    for name, value in enum:
        assert getattr(engine, "STATUS_" + name) == int(value), name
        assert getattr(pkg, "STATUS_" + name) == int(value), name


def test_rng_domains_named_once():
    dev = sources()["ddz_device.h"]
    body = re.search(r"enum RngDomain[^{]*\{(.*?)\};", dev, re.S).group(1)
    enum = re.findall(r"\bRNG_([A-Z_]+) = (\d+)", body)
    assert [n for n, _ in enum] == RNG
    assert [int(v) for _, v in enum] == list(range(1, 9))
    assert len({v for _, v in enum}) == 8


def test_no_status_literal_in_the_kernels():
    sites = 0
    for name, text in sources().items():
        for m in re.finditer(r"\batomicOr\(\s*((?:\w+(?:\.|->))?status)\s*,", text):
            arg = call_text(text, m.start())[1:-1].split(",", 1)[1]
            assert not re.search(r"(?<![\w.])\d", arg), (name, arg)
            sites += 1
            if arg.strip() == "bits":      # a computed word: the expression that makes it takes names too
                made = text[:m.start()].rsplit("bits =", 1)[1].split(";", 1)[0]
                assert "DDZ_ST_" in made and not re.search(r"(?<![\w.])[1-9]", made), (name, made)
    assert sites >= 48


def test_no_domain_literal_in_a_counter():
    helper = 0
    for name, text in sources().items():
        for m in re.finditer(r"make_uint4\(\(uint32_t\)g\w*, \(uint32_t\)\(g\w* >> 32\)", text):
            counter = call_text(text, m.start())
            assert not re.search(r"\du? << 16", counter), (name, counter)
            if name == "ddz_device.h" and "(uint32_t)domain << 16" in counter:
                helper += 1
            else:       # written out where the call compiled to other code: the domain still by its name
                assert re.search(r"\bRNG_[A-Z_]+ << 16", counter), (name, counter)
    assert helper == 1


def test_fresh_deal_meta_stated_once():
    text = "\n".join(sources().values())
    assert text.count("1u | (0xFFu << 16)") == 1
