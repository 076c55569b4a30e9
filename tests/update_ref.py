"""Pure-Python reference of the update audit's arithmetic (big integers), used only by tests.
TEST INFRASTRUCTURE ONLY.

  pack7          convert_byte_vec_to_field_elements_vec (fields.rs:109-112, data_field.rs:38-46):
                 7 little-endian bytes per element, the last zero padded; the RAW limbs
  horner         evaluate_field_polynomial_at_point_with_elevated_degree (fields.rs:172-186) over
                 canonical integers
  file_value     the file polynomial's canonical value: the raw limbs are Montgomery words, so
                 coefficient i is limb_i / R
  update_rows    the row-range rule of lcpc_pos_update_rows
  expected_difference   what an update changes in the file polynomial's value
"""
from __future__ import annotations

from pyref import Field

F63 = Field(0)
P = F63.p


def pack7(data: bytes) -> list:
    return [int.from_bytes(data[i:i + 7], "little") for i in range(0, len(data), 7)]


def horner(coeffs, x: int, degree_offset: int = 0, p: int = P) -> int:
    """sum_i coeffs[i] x^(i + degree_offset) mod p; x^0 = 1 also for x = 0."""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc * pow(x, degree_offset, p) % p


def naive(coeffs, x: int, degree_offset: int = 0, p: int = P) -> int:
    return sum(c * pow(x, i + degree_offset, p) for i, c in enumerate(coeffs)) % p


def file_value(data: bytes, x: int, degree_offset: int = 0) -> int:
    """Canonical value of the file polynomial of `data` at canonical x, elevated by degree_offset."""
    return horner(pack7(data), x, degree_offset) * pow(F63.R, -1, P) % P


def update_rows(old_len: int, offset: int, length: int, pre: int):
    """(row_lo, row_hi, old_lo, old_hi), or None where the library answers INVALID_ARG."""
    if length == 0 or offset > old_len or pre == 0:
        return None
    rb = 7 * pre
    row_lo, row_hi = offset // rb, (offset + length - 1) // rb + 1
    return row_lo, row_hi, min(row_lo * rb, old_len), min(row_hi * rb, old_len)


def apply_update(old: bytes, offset: int, data: bytes) -> bytes:
    buf = bytearray(old) + bytes(max(0, offset + len(data) - len(old)))
    buf[offset:offset + len(data)] = data
    return bytes(buf)


def expected_difference(old: bytes, offset: int, data: bytes, pre: int, x: int) -> int:
    """value(new file) - value(old file) from the touched rows alone."""
    row_lo, row_hi, old_lo, old_hi = update_rows(len(old), offset, len(data), pre)
    new = apply_update(old, offset, data)
    new_hi = min(row_hi * 7 * pre, len(new))
    d = row_lo * pre
    return (file_value(new[old_lo:new_hi], x, d) - file_value(old[old_lo:old_hi], x, d)) % P
