"""Writes tests/golden/cli_golden.json: what the REFERENCE's front-end prints, for tests/test_cli_report.py.

Needs a checkout of the reference project (REF: the directory whose src/ holds its main.cpp):

    python tests/golden/make_golden_cli.py REF

Output keys:
  report_literals  the string literals of the std::cout statements of main.cpp's reports, in the order the test's program calls
                   them (:469 scene, :512-515 grid, :523-533 memory, :439-444 benchmark), escapes resolved
  usage            the text of main.cpp's usage() up to its first std::endl, escapes resolved
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _cout_literals(text):
    """The string literals of the std::cout statements in `text`, in order."""
    out = []
    for stmt in re.findall(r"std::cout\s*<<(.*?);", text, flags=re.S):
        out += re.findall(r'"((?:[^"\\]|\\.)*)"', stmt)
    return [s for s in out if s.strip()]


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/make_golden_cli.py REF")
    ref = sys.argv[1]
    src = open(os.path.join(ref, "src", "main.cpp")).read()
    lines = src.split("\n")
    pick = lambda a, b: "\n".join(lines[a - 1:b])
    lits = _cout_literals(pick(469, 469)) + _cout_literals(pick(512, 515)) + _cout_literals(pick(523, 533)) + _cout_literals(pick(439, 444))
    body = src[src.index("static void usage()"):]
    body = body[:body.index("<< std::endl")]
    usage = "".join(s.encode().decode("unicode_escape") for s in re.findall(r'"((?:[^"\\]|\\.)*)"', body))
    out = {"report_literals": [l.encode().decode("unicode_escape") for l in lits], "usage": usage}
    with open(os.path.join(HERE, "cli_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote cli_golden.json: {len(lits)} literals, usage of {usage.count(chr(10))} lines")


if __name__ == "__main__":
    main()
