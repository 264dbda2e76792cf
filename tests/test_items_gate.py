"""The gate of the blocked g-SpMM's item kernels (csrc/gspmm_items.hip,
items_kernel, through the query dglhip_gspmm_items_kernel): which launches
take one item per wave (0), two (1, gspmm_items_pair_kernel) or four over a
column half (2, gspmm_items_columns_kernel).

The three kernels give the same bits, so no output comparison sees a gate that
wrongly declines; and the gate's size edges (a table or an output of 4 GiB)
are out of a quick GPU test's reach. This table is the only check of it. It
runs on the host: the addresses are made-up integers, nothing is dereferenced.

The expected values were read by hand from the two predicates and the dispatch
of the commit before the gate became a function of its own (488168f), where the
item kernels sat behind the generic sum dispatch:

* csrc/gspmm.hip 450-464 (dispatch_msg_layout) and csrc/gspmm_impl.h 953-971
  (launch_sum's POL_OK branch): only the instantiation <2, 64, COPY_U,
  EM_SCALAR, MEAN = false> asked the predicates, so copy_u over bf16 rows,
  u_mul_e and copy_e never reached them: the message rows.
* csrc/gspmm_impl.h 878-884 (items_pair_applies): items_per_wave == 2,
  F == 128, urows > 0, ldu % 4 == 0 (ldu 0 meaning F), ufeat % 16 == 0,
  out % 16 == 0, urows * ldu * 4 < 2^32: the F, urows, ldu, address,
  items_per_wave rows and the table rows at and past 2^32.
* csrc/gspmm_impl.h 891-896 (items_columns_applies): column_parts == 2, the
  above, urows * ldu * 4 <= 0xfffffc00, orows > 0, orows * F * 4 < 2^32: the
  column_parts and orows rows and the table rows around 0xfffffc00.

A table is urows * ldu * 4 bytes with ldu a multiple of 4, so a multiple of 16
bytes: the first size past 0xfffffc00 that the gate can be asked about is 16
bytes more, not 4 (a stride that is no multiple of 4 is declined for that
reason alone, the ldu 130 row).
"""
import ctypes

import pytest

COPY_U, U_MUL_E, COPY_E, COPY_U_BF16 = 0, 1, 2, 3
UFEAT = 0x7F0000000000  # made-up addresses, 16-byte aligned
OUT = 0x7E0000000000

#        msg, F, ldu, urows, orows, items_per_wave, column_parts, ufeat, out
BASE = dict(msg=COPY_U, F=128, ldu=0, urows=1000, orows=1000, items_per_wave=2, column_parts=2,
            ufeat=UFEAT, out=OUT)

ROWS = [
    ("base", {}, 2),
    # message
    ("copy_u bf16", dict(msg=COPY_U_BF16), 0),
    ("u_mul_e", dict(msg=U_MUL_E), 0),
    ("copy_e", dict(msg=COPY_E), 0),
    # F
    ("F 64", dict(F=64), 0),
    ("F 256", dict(F=256), 0),
    # urows
    ("urows unknown", dict(urows=0), 0),
    # ldu
    ("ldu 128", dict(ldu=128), 2),
    ("ldu 132", dict(ldu=132), 2),
    ("ldu 130", dict(ldu=130), 0),
    # addresses
    ("ufeat % 16 == 8", dict(ufeat=UFEAT + 8), 0),
    ("out % 16 == 8", dict(out=OUT + 8), 0),
    # table bytes = urows * ldu * 4
    ("table 0xfffffc00", dict(urows=8388606, ldu=128), 2),       # 8388606 * 512
    ("table 0xfffffc10", dict(urows=143779, ldu=7468), 1),       # 16 bytes more
    ("table 2^32 - 512", dict(urows=8388607, ldu=128), 1),       # one row more
    ("table 2^32 - 16", dict(urows=2113665, ldu=508), 1),        # the last below 4 GiB
    ("table 2^32", dict(urows=8388608, ldu=128), 0),
    ("table 2^32 + 512", dict(urows=8388609, ldu=128), 0),
    # out bytes = orows * 512
    ("orows unknown", dict(orows=0), 1),
    ("out 2^32 - 512", dict(orows=8388607), 2),
    ("out 2^32", dict(orows=8388608), 1),
    # items_per_wave
    ("items_per_wave 1, column_parts 2", dict(items_per_wave=1), 0),
    ("items_per_wave 1, column_parts 1", dict(items_per_wave=1, column_parts=1), 0),
    # column_parts
    ("column_parts 1", dict(column_parts=1), 1),
]


def test_table_sizes_are_what_the_rows_say():
    """The arithmetic of the rows' names (their edges are the point)."""
    sizes = {name: (BASE | ch)["urows"] * ((BASE | ch)["ldu"] or (BASE | ch)["F"]) * 4
             for name, ch, _ in ROWS if name.startswith("table ")}
    assert sizes == {"table 0xfffffc00": 0xFFFFFC00, "table 0xfffffc10": 0xFFFFFC10,
                     "table 2^32 - 512": 2**32 - 512, "table 2^32 - 16": 2**32 - 16,
                     "table 2^32": 2**32, "table 2^32 + 512": 2**32 + 512}
    assert all(((BASE | ch)["ldu"] % 4 == 0) for name, ch, _ in ROWS if name.startswith("table "))


@pytest.mark.parametrize("name,change,expected", ROWS, ids=[r[0] for r in ROWS])
def test_items_gate(name, change, expected):
    from dgl import _ffi
    a = BASE | change
    kernel = ctypes.c_int(-1)
    _ffi.check_call(_ffi.LIB.dglhip_gspmm_items_kernel(
        a["msg"], a["F"], a["ldu"], a["urows"], a["orows"], a["items_per_wave"],
        a["column_parts"], a["ufeat"], a["out"], ctypes.addressof(kernel)))
    assert kernel.value == expected
