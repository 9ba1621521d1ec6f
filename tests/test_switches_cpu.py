"""The run-time switches of the package and the table that documents them ("Run-time switches") name the same
environment variables: a switch that is added without a row, or a row whose switch is gone, fails here.  A plain text scan."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")

# "MIS_X" handed to getenv(...) / os.environ.get(...) / os.environ[...] / ... in os.environ
READ = re.compile(r'(?:getenv\s*\(\s*|environ\s*(?:\.\s*(?:get|setdefault|pop)\s*\(|\[)\s*)["\'](MIS_[A-Z0-9_]+)["\']')
MEMBER = re.compile(r'["\'](MIS_[A-Z0-9_]+)["\']\s+(?:not\s+)?in\s+(?:\w+\.)?environ')


def switches_read():
    names = {}
    for top, _, files in os.walk(PKG):
        for f in files:
            if not f.endswith((".py", ".hip", ".h", ".inc")):
                continue
            path = os.path.join(top, f)
            with open(path, encoding="utf-8", errors="replace") as fh:
                text = fh.read()
            for m in list(READ.finditer(text)) + list(MEMBER.finditer(text)):
                names.setdefault(m.group(1), os.path.relpath(path, ROOT))
    return names


def switches_documented():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        text = fh.read()
    section = re.search(r"^## Run-time switches$(.*?)(?=^## )", text, re.M | re.S)
    assert section, "DESIGN.md has no 'Run-time switches' section"
    return set(re.findall(r"^\| `(MIS_[A-Z0-9_]+)` \|", section.group(1), re.M))


def test_the_switch_table_lists_what_the_code_reads():
    read, documented = switches_read(), switches_documented()
    assert len(read) >= 20 and "MIS_GEMM_BF3" in read and "MIS_WINO" in read, sorted(read)      # the scan sees both languages
    missing = {n: read[n] for n in read if n not in documented}
    stale = sorted(documented - set(read))
    assert not missing, f"read by the code, no row in DESIGN.md 'Run-time switches': {missing}"
    assert not stale, f"rows of DESIGN.md 'Run-time switches' that nothing reads: {stale}"
