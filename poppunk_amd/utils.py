"""Mirrors of the PopPUNK/utils.py helpers that sit on the distance path.

`update_distance_matrices` (PopPUNK/utils.py:357-408) is what `poppunk_assign --update-db` and the
visualisation code use to merge the stored ref-ref distances with freshly computed query-ref and
query-query distances: three long-form matrices -> two (n_ref + n_query)^2 square matrices.  The reference
slices each column out on the host and converts it by itself (`pp_sketchlib.longToSquare[Multi]`, which stay
available in `poppunk_amd.pp_sketchlib` for PopPUNK's own copy of this function); here both squares come from
one engine call on the two-column matrices (`ppk_long_to_square2`, ppk_square.hip).  The file
helpers (`storePickle`, `readPickle`, utils.py:135-196), the row iterator (`iterDistRows`,
utils.py:199-226) and the fd-level `stderr_redirected` (utils.py:61-83) live here too, so that
`from poppunk_amd.utils import ...` reads like the reference's import lines.
"""
import os
import sys
from contextlib import contextmanager

import numpy as np

from . import pp_sketchlib
from .distfile import readPickle, storePickle  # noqa: F401


@contextmanager
def stderr_redirected(to=os.devnull):
    """Everything written to FILE DESCRIPTOR 2 inside the block -- Python's sys.stderr and native code
    alike -- goes to `to` (PopPUNK/utils.py:61-83, used around the --plot-fit re-queries to hide their
    progress meters, PopPUNK/sketchlib.py:546).  libppk_hip.so writes its meter with write(2), so this
    silences it."""
    fds = [2]                                   # what native code writes to
    try:
        if sys.stderr.fileno() not in fds:      # a re-pointed sys.stderr (test harnesses, wrappers)
            fds.append(sys.stderr.fileno())
    except (AttributeError, OSError, ValueError):
        pass
    try:
        sys.stderr.flush()
    except Exception:
        pass
    saved = [os.dup(fd) for fd in fds]
    try:
        with open(to, "w") as sink:
            for fd in fds:
                os.dup2(sink.fileno(), fd)
        yield
    finally:
        try:
            sys.stderr.flush()
        except Exception:
            pass
        for fd, old in zip(fds, saved):
            os.dup2(old, fd)
            os.close(old)


def readIsolateTypeFromCsv(clustCSV, mode='clusters', return_dict=False):
    """Cluster definitions from a CSV file (PopPUNK/utils.py:264-319), read with the csv module (pandas is not a
    dependency of this package).  The first column names the samples; the other columns are selected by `mode`:
    'clusters' (columns with 'Cluster' in their name), 'lineages' ('Rank_' or 'overall'), 'external' (the only column,
    or every column but the last).  Returns {column: {cluster: set of samples}}, or with return_dict
    {column: {sample: cluster}}; '__autocolour' is dropped from column names.  Every value is the cell's text: the
    reference's pandas reads an all-numeric column as numbers first, so '07' becomes '7' there and stays '07' here,
    and numeric sample names are ints in its sets."""
    import csv
    with open(clustCSV, newline='') as f:
        table = [row for row in csv.reader(f, quotechar='"') if row]
    header = [col.replace('__autocolour', '') for col in table[0][1:]] if table else []
    wanted = {'clusters': lambda k, col: 'Cluster' in col,
              'lineages': lambda k, col: 'Rank_' in col or 'overall' in col,
              'external': lambda k, col: k == 0 if len(header) == 1 else k < len(header) - 1}
    if mode not in wanted:
        sys.stderr.write('Unknown CSV reading mode: ' + mode + '\n')
        sys.exit(1)
    # the column test sees the name as the file has it ('__autocolour' and all), the result carries it stripped
    picked = [k for k, col in enumerate(table[0][1:] if table else []) if wanted[mode](k, col)]
    out = {}
    for sample, *cells in table[1:]:
        for k in picked:
            column = out.setdefault(header[k], {})
            if return_dict:
                column[sample] = cells[k]
            else:
                column.setdefault(cells[k], set()).add(sample)
    return out


def isolateNameToLabel(names):
    """Sample names as labels (PopPUNK/utils.py:473-488): what follows the last '/', '.' '(' ')' as '_', ':' dropped."""
    drop = str.maketrans({'.': '_', ':': None, '(': '_', ')': '_'})
    return [name.split('/')[-1].translate(drop) for name in names]


def readRfile(rFile, oneSeq=False):
    """The list of assemblies to sketch (PopPUNK/utils.py:410-471): one sample per line, its name and its sequence
    file(s) separated by tabs.  Returns (names, sequences) sorted by name, `sequences[i]` the list of files of sample i
    (with oneSeq its first file alone, with the reference's note when there are more).  A line with fewer than two
    fields, a '/' in a name and duplicate names (after isolateNameToLabel) each write the reference's message to stderr
    and exit(1)."""
    names, sequences = [], []
    with open(rFile, 'r') as listing:
        for line in listing:
            fields = line.rstrip().split("\t")
            if len(fields) < 2:
                sys.stderr.write("Input reference list is misformatted\n"
                                 "Must contain sample name and file, tab separated\n")
                sys.exit(1)
            if "/" in fields[0]:
                sys.stderr.write("Sample names may not contain slashes\n")
                sys.exit(1)
            names.append(fields[0])
            if oneSeq:
                if len(fields) > 2:
                    sys.stderr.write("Multiple sequence found for " + fields[0] + ". Only using first\n")
                sequences.append(fields[1])
            else:
                sequences.append(fields[1:])
    names = isolateNameToLabel(names)
    if len(set(names)) != len(names):
        seen, dupes = set(), set()
        for name in names:
            (dupes if name in seen else seen).add(name)
        sys.stderr.write("Input contains duplicate names! All names must be unique\n")
        sys.stderr.write("Non-unique names are " + ",".join(dupes) + "\n")
        sys.exit(1)
    # sorted by name on return, as the reference does (an empty list stays two empty lists)
    order = sorted(range(len(names)), key=lambda i: (names[i], sequences[i]))
    return [names[i] for i in order], [sequences[i] for i in order]


def iterDistRows(refSeqs, querySeqs, self=True):
    """Row -> (ref, query) names of the distance matrix (PopPUNK/utils.py:199-226)."""
    if self:
        if refSeqs != querySeqs:
            raise RuntimeError('refSeqs must equal querySeqs for db building (self = true)')
        for i, ref in enumerate(refSeqs):
            for j in range(i + 1, len(refSeqs)):
                yield (refSeqs[j], ref)
    else:
        for query in querySeqs:
            for ref in refSeqs:
                yield (ref, query)


def update_distance_matrices(refList, distMat, queryList=None, query_ref_distMat=None,
                             query_query_distMat=None, threads=1):
    """Long form (n_comparisons x 2: core, accessory) -> the two square matrices, merging query distances when
    a query list is given: (seqLabels, coreMat, accMat), the contract of PopPUNK/utils.py:357-408.  Both squares
    come from ONE engine call on the two-column matrices as they are (`pp_sketchlib.squareMatrices` ->
    `ppk_long_to_square2`: each matrix crosses PCIe once and the kernels read its columns in place); `threads` is
    accepted for the signature and unused."""
    if queryList is None:
        core, acc = pp_sketchlib.squareMatrices(distMat)
        return refList, core, acc
    core, acc = pp_sketchlib.squareMatrices(distMat, query_ref_distMat, query_query_distMat)
    return refList + queryList, core, acc


def transformLine(s, mean0, mean1):
    """The point at distance s from mean0 along the line mean0 -> mean1 (PopPUNK/utils.py:509-532), as
    np.array([x, y]).  The statement order is the reference's: every caller compares doubles derived from it."""
    dx = mean1[0] - mean0[0]
    dy = mean1[1] - mean0[1]
    ds = np.sqrt(dx**2 + dy**2)
    x = mean0[0] + s * (dx / ds)
    y = mean0[1] + s * (dy / ds)
    return np.array([x, y])


def decisionBoundary(intercept, gradient, adj=0.0):
    """The axis intercepts (x, y) of the boundary through `intercept`, normal to a line of slope `gradient`
    (PopPUNK/utils.py:535-560).  With adj != 0 the point is first moved along its own direction from the origin by
    adj, IN PLACE as the reference does it: refineFit's unconstrained branch passes mean0 and mean1 themselves and goes
    on with the moved points."""
    if adj != 0.0:
        original_hypotenuse = (intercept[0]**2 + intercept[1]**2)**0.5
        length_ratio = (original_hypotenuse + adj) / original_hypotenuse
        intercept[0] = intercept[0] * length_ratio
        intercept[1] = intercept[1] * length_ratio
    x = intercept[0] + intercept[1] * gradient
    y = intercept[1] + intercept[0] / gradient
    return (x, y)
