"""Imputed dosages on the host: expected allele counts in [0, 2], as BGEN / pgen / VCF ``DS`` readers hand them out, in the two
element types the device path takes.  Nothing here needs a GPU or the built library.

``float32``: the value itself, NaN (any non-finite value) = missing.  ``uint16``: PLINK 2's fixed point, ``DOSAGE_ONE`` = 16384
codes per allele, so 32768 = 2.0; any code above 32768 is missing, ``DOSAGE_MISSING`` = 65535 is the canonical one.  The fixed
point is the compact exact form: its moments are integer sums on the device, and a hard call ``g`` coded ``g * 16384`` gives
the bits of the int8 path.

    codes = dosage.encode(ds)                          # m x N float -> uint16, NaN -> 65535
    out = scan.scan_dosages(codes, sample_index=idx)   # scilmm_amd.assoc.AssociationScan
    out = scan.scan_dosages(ds.astype(np.float32))     # ... or the floats as they are
"""
import numpy as np

DOSAGE_ONE = 16384
DOSAGE_MISSING = 65535


def encode(d):
    """Dosages (any float array, NaN = missing) as uint16 codes ``rint(d * 16384)``, NaN -> 65535.  ValueError for a value
    that is not NaN and not in [0, 2]."""
    d = np.asarray(d, dtype=np.float64)
    miss = np.isnan(d)
    with np.errstate(invalid="ignore"):
        if np.any(~miss & ~((d >= 0.0) & (d <= 2.0))):
            raise ValueError("a dosage outside [0, 2]: only NaN stands for a missing value")
    codes = np.full(d.shape, DOSAGE_MISSING, dtype=np.uint16)
    codes[~miss] = np.rint(d[~miss] * DOSAGE_ONE).astype(np.uint16)
    return codes


def decode(codes):
    """uint16 codes as float64 dosages, NaN for every missing code (above 32768)."""
    codes = np.asarray(codes)
    if codes.dtype != np.uint16:
        raise TypeError("codes must be uint16, got %s" % codes.dtype)
    out = codes.astype(np.float64) / DOSAGE_ONE
    out[codes > 2 * DOSAGE_ONE] = np.nan
    return out


def check_dosages(d, N=None):
    """The dosage matrix as the device path takes it: m x N, marker-major, C-contiguous (``np.memmap`` included), uint16
    codes or float32 values; ``N`` = None accepts any number of columns.  TypeError for another type or dtype, ValueError for
    another shape or layout; nothing is converted or copied here."""
    if not isinstance(d, np.ndarray):
        raise TypeError("dosages must be a NumPy uint16 or float32 array (np.memmap included), got %s" % type(d).__name__)
    if d.dtype == np.float64:
        raise TypeError("dosages must be float32 or uint16 codes, got float64: pass d.astype(np.float32), or the compact "
                        "exact form scilmm_amd.dosage.encode(d)")
    if d.dtype not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise TypeError("dosages must be uint16 codes (16384 = one allele) or float32 values, got %s" % d.dtype)
    if d.ndim != 2:
        raise ValueError("dosages must be 2-D, markers x samples; got %d-D" % d.ndim)
    if N is not None and d.shape[1] != N:
        raise ValueError("dosages have %d columns, %d samples are expected" % (d.shape[1], N))
    if not d.flags.c_contiguous:
        raise ValueError("dosages must be C-contiguous (marker-major)")
    return d
