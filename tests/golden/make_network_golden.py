"""Convert the reference's reactor-network golden result files into JSON fixtures.

    python make_network_golden.py <directory of the reference's tests/baseline>

Same conversion as make_golden.py (the .baseline files are Python dict literals produced by the licensed Chemkin):
ast.literal_eval -> json.dump.  Only the data values are kept; the inputs that produced them are restated in
tests/network_cases.py with the reference script file:line they come from.
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("PSRnetwork", "PSRChain_network", "PSRChain_declustered")

if __name__ == "__main__":
    src = sys.argv[1]
    for name in NAMES:
        with open(os.path.join(src, name + ".baseline")) as f:
            d = ast.literal_eval(f.read())
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump(d, f, indent=0)
        print(name, sorted(d))
