"""The table type of the stream-order case tables and the parser of the headers they are held against (a plain helper
module, standard library only: imports without a GPU and without the package).

One Table per header of include/ that declares entry points taking a `qi_stream`: tests/stream_cases.py for qi_tfr.h and one
satellite module per array header.  A case names the functions it reaches and builds, on the device, a closure
`op(x) -> tuple of device tensors` together with two record sets A and B of one shape (Built); tests/stream_order.py runs it.
Besides its cases a table declares, as data, what the harness does with them:

    complex_input  the record pair is uploaded as [..., 2] (re, im) values and handed to the closure through view_as_complex
    power          which outputs must differ between op(A) and op(B) for a case to have power: "any" of them, output "first"
                   (and then the result behind the producer differs from the stale one exactly where the serial ones do) or
                   "every" output (and then so does the result behind the producer)
    finite         every serial output is finite
    no_fill        no serial output holds the closures' fill value
    zero_outputs   {case id: index of an output, such as `info`, that is zero on both record sets}

The census of a table against its header is in the header's CPU test, through header_functions and stream_functions.
"""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# engine: the key of the plan a plan case runs on, None for a plan-less case -- the two groups of the host-thread tests
# (tests/test_gpu_threads.py): a plan belongs to one thread at a time, a plan-less op may be called from several at once
Case = collections.namedtuple("Case", "id functions asynchronous reason build engine")
Built = collections.namedtuple("Built", "op a b note")  # a, b: NumPy record sets; note: what the build asserted, for the log
POWER_RULES = ("any", "first", "every")


class Table:
    Case, Built = Case, Built

    def __init__(self, header, complex_input=False, power="any", finite=False, no_fill=False, zero_outputs=None):
        assert header.startswith("qi_") and header.endswith(".h") and power in POWER_RULES, (header, power)
        self.header, self.name = header, header[3:-2]  # qi_lags.h -> lags: the prefix of the test ids
        self.complex_input, self.power, self.finite, self.no_fill = complex_input, power, finite, no_fill
        self.zero_outputs = dict(zero_outputs or {})
        self.cases = []

    def case(self, cid, functions, build, asynchronous=True, reason="", engine=None):
        assert asynchronous or reason, cid
        assert cid not in self.ids(), cid
        self.cases.append(Case(cid, tuple(functions), asynchronous, reason, build, engine))

    def ids(self):
        return [c.id for c in self.cases]

    def by_id(self, cid):
        return next(c for c in self.cases if c.id == cid)

    def named_functions(self):
        return sorted({f for c in self.cases for f in c.functions})

    def plan_less_ids(self):
        return [c.id for c in self.cases if c.engine is None]


def header_functions(header):
    """{name: parameter text} of every function include/<header> declares (comments removed first)."""
    with open(os.path.join(ROOT, "include", header)) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    return dict(re.findall(r"\b(qi_\w+)\s*\(([^;{}()]*)\)\s*;", text))


def stream_functions(header):
    return sorted(name for name, params in header_functions(header).items() if re.search(r"\bqi_stream\b", params))
