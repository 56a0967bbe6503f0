"""CPU: the table of environment variables in DESIGN.md ("Environment variables") lists exactly
the SBAG_* names that the library's sources read with getenv.  A variable added to the library
needs a row there, with what it does and when it is read; one whose row goes, goes from the
sources too.  Reads source text for these names only."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "spark-bagging_amd", "csrc")


def names_read_by_library():
    names = set()
    for pat in ("*.hip", "*.cpp", "*.h"):
        for path in glob.glob(os.path.join(CSRC, pat)):
            with open(path) as f:
                # every SBAG_ string literal inside a getenv(...) call (one call chooses
                # between two names with ?:)
                for call in re.findall(r"getenv\(([^()]*)\)", f.read()):
                    names |= set(re.findall(r'"(SBAG_[A-Z0-9_]+)"', call))
    return names


def names_in_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text.split("### Environment variables", 1)[1].split("\n## ", 1)[0]
    return re.findall(r"^\| `(SBAG_[A-Z0-9_]+)` \|", section, flags=re.M)


def test_table_lists_every_variable_the_library_reads():
    table = names_in_table()
    assert len(table) == len(set(table)), "a variable has two rows"
    read = names_read_by_library()
    assert read, "no getenv(\"SBAG_...\") found: the search is broken"
    assert set(table) == read, {"read but not in the table": sorted(read - set(table)),
                                "in the table but not read": sorted(set(table) - read)}
