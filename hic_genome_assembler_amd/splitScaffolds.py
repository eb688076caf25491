"""Cut scaffolds at chosen bases and rebuild every input of the pipeline for the broken assembly.

``supportSpans -cuts FILE`` says after which base a scaffold should be cut; nothing acted on that file.  This tool takes a
config and a list of cuts and writes a complete, runnable input set for the assembly with the cut scaffolds replaced by
their pieces: the size file, an AGP, the FASTA, the restriction sites, the valid pairs, the order file, and per resolution
the raw and balanced contact map with a config for ``-part1 ... -part4``.  The map from a read end (scaffold, position) to
(piece, position in the piece) is applied to every pair of ``validPairFile`` on the device before the pair is counted
(``hicmi_split_maps``: one pass over the file for all resolutions and the per-piece counters), and again on the host when
the pair file is rewritten (``hicmi_split_valid_pairs``).

    python -m hic_genome_assembler_amd.splitScaffolds -config my_config.txt -cuts FILE [-resolution 100000,250000] \\
           [-order FILE] [-minPiece 1] [-out DIR] [-noBalance] [-noPairs] [-threads 0] [-device 0]

Cuts file: tab-separated ``scaffold  cut_after [anything more]`` lines, ``#`` lines and blank lines skipped; ``cut_after = c``
parts the bases 1 .. c from c + 1 .. L.  A scaffold with k kept cuts becomes ``NAME.brk1 .. NAME.brk(k+1)``, left to right,
in the parent's place in the size file; an uncut scaffold keeps its name.  In ``DIR`` (``saveFilesDirectory/split``):
``split.sizes``, ``split.agp``, ``split.fasta`` (when ``originalFastaFile`` is a file), ``split.restriction.bed`` (when
``restrictionSiteFile`` is a file), ``split.allValidPairs`` (unless ``-noPairs``), the order file under its own base name
(when one is given or found), ``res<r>/`` per resolution and ``split_summary.tsv``.  ``chromosomeGroupFile`` is not carried
over: its bin IDs belong to the old bed file.
"""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib
from .assembledMap import set_config_values
from .buildMap import MAX_BINS, STATS_COLUMNS, SUMMARY_COLUMNS, check_valid_pair_file, parse_resolutions
from .hostio import bins_from_sizes, count_bins, paused_gc, read_scaffold_sizes
from .rebinMap import output_paths, scaffold_counts, write_resolution
from .writeAssembledFasta import readFastaIntoMem, writeSeqToFile

PIECE_SUFFIX = ".brk"                            # supportBreaks' suffix
PIECE_COLUMNS = ("piece", "parent", "first_base", "last_base", "size", "within", "sibling", "other", "spanning")


@dataclass
class Pieces:
    """The pieces of a cut assembly and the tables of DESIGN.md 9o."""
    names: list                     # piece names, in the size file's order with every cut scaffold replaced by its pieces
    sizes: np.ndarray               # int64[n_piece]
    parent: np.ndarray              # int32[n_piece]  index of the parent in the size file
    piece_first: np.ndarray         # int32[S + 1]
    piece_start: np.ndarray         # int64[n_piece]  bases of the parent before the piece
    applied: dict                   # parent name -> kept cuts, ascending
    skipped: list                   # (parent name, cut) that -minPiece dropped


def parse_cuts(cutsFile):
    """{scaffold: cuts ascending, repeats merged} of a cuts file.  ValueError for a line without a second column and for a
    ``cut_after`` that is not an integer."""
    cuts = {}
    with open(cutsFile) as fh:
        for number, line in enumerate(fh, 1):
            body = line.rstrip("\r\n")
            if not body.strip() or body.startswith("#"):
                continue
            cols = body.split("\t")
            if len(cols) < 2:
                raise ValueError("line %d of %s has no cut_after column" % (number, cutsFile))
            try:
                c = int(cols[1].strip())
            except ValueError:
                raise ValueError("line %d of %s: cut_after %r is not an integer" % (number, cutsFile, cols[1]))
            cuts.setdefault(cols[0], set()).add(c)
    return {name: sorted(cs) for name, cs in cuts.items()}


def make_pieces(names, sizes, cuts, min_piece=1):
    """The pieces of the scaffolds (names, sizes) cut at ``cuts`` (parse_cuts).  Cuts of a scaffold are taken in ascending
    order; one closer than ``min_piece`` bases to the previously kept cut or to either end of the scaffold is skipped.
    ValueError for a scaffold the size file does not have, a cut below 1 or at or beyond the size, a ``min_piece`` below 1
    and a piece name the size file already has."""
    min_piece = int(min_piece)
    if min_piece < 1:
        raise ValueError("minPiece %d is below 1" % min_piece)
    index = {name: s for s, name in enumerate(names)}
    for name, cs in cuts.items():
        if name not in index:
            raise ValueError("scaffold %s of the cuts file is not in the scaffold size file" % name)
        L = int(sizes[index[name]])
        for c in cs:
            if c < 1 or c >= L:
                raise ValueError("cut_after %d of scaffold %s is outside 1 .. %d (its size less one)" % (c, name, L - 1))
    out_names, out_sizes, parent, first, start, applied, skipped = [], [], [], [0], [], {}, []
    for s, name in enumerate(names):
        L, kept = int(sizes[s]), []
        for c in sorted(set(cuts.get(name, ()))):
            if c - (kept[-1] if kept else 0) < min_piece or L - c < min_piece:
                skipped.append((name, c))
            else:
                kept.append(c)
        bounds = [0] + kept + [L]
        if kept:
            applied[name] = kept
        for k in range(len(bounds) - 1):
            out_names.append("%s%s%d" % (name, PIECE_SUFFIX, k + 1) if kept else name)
            out_sizes.append(bounds[k + 1] - bounds[k])
            parent.append(s)
            start.append(bounds[k])
        first.append(len(out_names))
    made = {n for n, p in zip(out_names, parent) if names[p] in applied}
    clash = sorted(made & set(names))
    if clash:
        raise ValueError("the piece name %s is already a scaffold of the size file" % clash[0])
    return Pieces(out_names, np.asarray(out_sizes, np.int64), np.asarray(parent, np.int32), np.asarray(first, np.int32),
                  np.asarray(start, np.int64), applied, skipped)


def sizes_text(pieces):
    """``split.sizes``: name and size of every piece, the format of hicProScaffSizeFile."""
    return "".join("%s\t%d\n" % ns for ns in zip(pieces.names, pieces.sizes.tolist()))


def agp_text(pieces, names):
    """``split.agp`` (AGP 2.0): one W line per piece, the object the piece, the component its parent with the 1-based range."""
    out = ["##agp-version\t2.0\n"]
    for name, size, p, start in zip(pieces.names, pieces.sizes.tolist(), pieces.parent.tolist(), pieces.piece_start.tolist()):
        out.append("%s\t1\t%d\t1\tW\t%s\t%d\t%d\t+\n" % (name, size, names[p], start + 1, start + size))
    return "".join(out)


def check_fasta(fasta, pieces, names, sizes):
    """ValueError when a cut scaffold is missing from the FASTA or has another length there than in the size file."""
    for s, name in enumerate(names):
        if name in pieces.applied:
            if name not in fasta:
                raise ValueError("scaffold %s is cut but is not in originalFastaFile" % name)
            if len(fasta[name]) != int(sizes[s]):
                raise ValueError("scaffold %s has %d bases in originalFastaFile and %d in the scaffold size file"
                                 % (name, len(fasta[name]), int(sizes[s])))


def write_fasta(path, fasta, pieces, names):
    """``split.fasta``: the entries of ``fasta`` in their order, a cut scaffold replaced by its pieces; Part 4's line width."""
    index = {name: s for s, name in enumerate(names)}
    with open(path, "w") as fh:
        for name, seq in fasta.items():
            if name in pieces.applied:
                s = index[name]
                for k in range(int(pieces.piece_first[s]), int(pieces.piece_first[s + 1])):
                    a = int(pieces.piece_start[k])
                    fh.write(">" + pieces.names[k] + "\n")
                    writeSeqToFile(fh, seq[a:a + int(pieces.sizes[k])])
            else:
                fh.write(">" + name + "\n")
                writeSeqToFile(fh, seq)


def restriction_text(lines, pieces, names):
    """The lines of a restriction site file moved to the pieces: a site of a cut scaffold goes to the piece that holds its
    column-3 coordinate (0: the first piece), columns 2 and 3 less the piece's start, column 2 not below 0; every other
    line verbatim.  ValueError for a site of a cut scaffold without an integer in columns 2 and 3."""
    index = {name: s for s, name in enumerate(names)}
    out = []
    for number, raw in enumerate(lines, 1):
        body = raw.rstrip("\r\n")
        cols = body.split("\t")
        if cols[0] not in pieces.applied:
            out.append(raw)
            continue
        try:
            lo, hi = int(cols[1]), int(cols[2])
        except (IndexError, ValueError):
            raise ValueError("line %d of restrictionSiteFile has no integers in columns 2 and 3" % number)
        s = index[cols[0]]
        first, last = int(pieces.piece_first[s]), int(pieces.piece_first[s + 1])
        k = first + max(int(np.searchsorted(pieces.piece_start[first:last], hi, side="left")) - 1, 0)
        at = int(pieces.piece_start[k])
        out.append("\t".join([pieces.names[k], str(max(lo - at, 0)), str(hi - at)] + cols[3:]) + raw[len(body):])
    return "".join(out)


def order_text(lines, pieces):
    """The lines of an order file with every cut parent replaced by its pieces: a ``+`` parent by brk1 .. brk(k+1), each
    ``+``, a ``-`` parent by brk(k+1) .. brk1, each ``-``; every other line verbatim.  ValueError for a cut parent with
    another orientation."""
    out = []
    for number, raw in enumerate(lines, 1):
        body = raw.rstrip("\r\n")
        cols = body.split("\t")
        if number == 1 or body.startswith("#") or cols[0] not in pieces.applied:
            out.append(raw)
            continue
        if len(cols) < 2 or cols[1] not in ("+", "-"):
            raise ValueError("line %d of the order file: the cut scaffold %s has no orientation + or -" % (number, cols[0]))
        end = raw[len(body):] or "\n"
        parts = ["%s%s%d" % (cols[0], PIECE_SUFFIX, k + 1) for k in range(len(pieces.applied[cols[0]]) + 1)]
        for part in (parts if cols[1] == "+" else parts[::-1]):
            out.append("\t".join([part] + cols[1:]) + end)
    return "".join(out)


def _is_real_file(path):
    return bool(path) and os.path.isfile(path) and not os.path.samefile(path, os.devnull)


class _Device:
    """The device calls of a run; a test hands runPipeline a stand-in with the same two methods."""

    def __init__(self, device):
        self.device = device

    def split_maps(self, path, names, sizes, piece_first, piece_start, resolutions, threads):
        """(stats5, counters uint64[4, n_piece], one context per resolution holding its raw map)."""
        ctxs = [_lib.Context(self.device) for _r in range(max(len(resolutions), 1))]
        try:
            stats, counters = _lib.split_maps(path, names, sizes, piece_first, piece_start, resolutions, ctxs, threads=threads)
        except BaseException:
            for ctx in ctxs:
                ctx.close()
            raise
        for ctx in ctxs[len(resolutions):]:
            ctx.close()
        return stats, counters, ctxs[:len(resolutions)]

    def split_valid_pairs(self, path_in, path_out, names, sizes, piece_first, piece_start, piece_names, threads):
        return _lib.split_valid_pairs(path_in, path_out, names, sizes, piece_first, piece_start, piece_names, threads=threads)


def runPipeline(configFile, cutsFile, resolutions=(), orderFile=None, minPiece=1, outDir=None, balance=True, pairs=True, threads=0,
                device=0, context=None):
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    ice = driver.iceSettings(v)
    resolutions = list(resolutions)
    if outDir is None:
        outDir = os.path.join(v["saveFilesDirectory"], "split")
    outDir = os.path.abspath(outDir)
    if orderFile is None:
        orderFile = next((v[key] for key in ("finalOrderingsFile", "chromosomeOrderFile") if os.path.isfile(v[key])), None)
    have_pairs = pairs or bool(resolutions)
    try:
        names, sizes = read_scaffold_sizes(v["hicProScaffSizeFile"])
        if not names:
            raise ValueError("hicProScaffSizeFile %s lists no scaffold" % v["hicProScaffSizeFile"])
        if not os.path.isfile(cutsFile):
            raise ValueError("cuts file %r does not exist" % cutsFile)
        pieces = make_pieces(names, sizes, parse_cuts(cutsFile), minPiece)
        if have_pairs:
            check_valid_pair_file(v["validPairFile"])
        elif _is_real_file(v["validPairFile"]):
            have_pairs = True                                       # the counters of the summary are still made
        for r in resolutions:
            m = count_bins(pieces.sizes, r)
            if m > MAX_BINS:
                raise ValueError("resolution %d needs %d bins, more than the %d a map can have" % (r, m, MAX_BINS))
        new_order = None
        if orderFile is not None:
            if not os.path.isfile(orderFile):
                raise ValueError("order file %r does not exist" % orderFile)
            with open(orderFile, newline="") as fh:
                new_order = order_text(fh.readlines(), pieces)
        new_sites = None
        if _is_real_file(v["restrictionSiteFile"]):
            with open(v["restrictionSiteFile"], newline="") as fh:
                new_sites = restriction_text(fh, pieces, names)
        fasta = None
        if _is_real_file(v["originalFastaFile"]):
            fasta = readFastaIntoMem(v["originalFastaFile"])
            check_fasta(fasta, pieces, names, sizes)
    except (OSError, ValueError) as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    dev = context if context is not None else _Device(device)
    n_piece = len(pieces.names)
    out = {"hicProScaffSizeFile": os.path.join(outDir, "split.sizes"), "validPairFile": os.devnull, "restrictionSiteFile": os.devnull,
           "originalFastaFile": os.devnull}
    rows, stats, counters, ctxs = [], None, None, []
    with paused_gc():
        try:
            if have_pairs:
                try:
                    # the first pass over the pair file: a malformed line ends the run before anything is written
                    stats, counters, ctxs = dev.split_maps(v["validPairFile"], names, sizes, pieces.piece_first, pieces.piece_start,
                                                           resolutions, threads)
                except _lib.HicmiError as exc:
                    sys.exit("ERROR... %s. Exiting..." % exc)
                print("SPLIT: lines %d, pairs used %d, unknown scaffold %d, out of range %d, chunks %d" % tuple(stats))
                if stats[3]:
                    print("WARNING... %d line(s) of %s have a position below 1 or beyond the size of their scaffold in %s and "
                          "were skipped: do the two files belong to one assembly?" % (stats[3], v["validPairFile"],
                                                                                      v["hicProScaffSizeFile"]))
            os.makedirs(outDir, exist_ok=True)
            if pairs:
                out["validPairFile"] = os.path.join(outDir, "split.allValidPairs")
                try:
                    dev.split_valid_pairs(v["validPairFile"], out["validPairFile"], names, sizes, pieces.piece_first, pieces.piece_start,
                                          pieces.names, threads)
                except _lib.HicmiError as exc:
                    sys.exit("ERROR... %s. Exiting..." % exc)
            with open(out["hicProScaffSizeFile"], "w") as fh:
                fh.write(sizes_text(pieces))
            with open(os.path.join(outDir, "split.agp"), "w") as fh:
                fh.write(agp_text(pieces, names))
            if fasta is not None:
                out["originalFastaFile"] = os.path.join(outDir, "split.fasta")
                write_fasta(out["originalFastaFile"], fasta, pieces, names)
                del fasta
            if new_sites is not None:
                out["restrictionSiteFile"] = os.path.join(outDir, "split.restriction.bed")
                with open(out["restrictionSiteFile"], "w", newline="") as fh:
                    fh.write(new_sites)
            if new_order is not None:
                with open(os.path.join(outDir, os.path.basename(orderFile)), "w", newline="") as fh:
                    fh.write(new_order)
            v_piece = dict(v, hicProScaffSizeFile=out["hicProScaffSizeFile"])     # iceMinScaffoldSize looks at the pieces
            for r, ctx in zip(resolutions, ctxs):
                binList = bins_from_sizes((pieces.names, pieces.sizes), r)
                paths = output_paths(outDir, r, prefix="split")
                n_scaf, n_one = scaffold_counts(binList)
                line = "SPLIT: resolution %d, bins %d (pieces %d, of one bin %d)" % (r, len(binList), n_scaf, n_one)
                ice_cols, n_pairs = write_resolution(ctx, binList, paths, configFile, v_piece, ice, balance, line)
                set_config_values(os.path.join(paths["dir"], "config.txt"), out)
                rows.append([str(r), str(len(binList)), str(n_scaf), str(n_one)] + ice_cols + [repr(n_pairs)])
                ctx.close()                                             # its map is written: the memory goes back now
        finally:
            for ctx in ctxs:
                ctx.close()
    spanning = _lib.split_spanning(pieces.piece_first, counters) if counters is not None else None
    last_of_parent = set((pieces.piece_first[1:] - 1).tolist())
    n_cuts = sum(len(c) for c in pieces.applied.values())
    with open(os.path.join(outDir, "split_summary.tsv"), "w") as fh:
        head = list(zip(STATS_COLUMNS, stats[:4])) if stats is not None else [(key, "NA") for key in STATS_COLUMNS]
        fh.write("#" + "\t".join("%s=%s" % kv for kv in head + [("cuts", n_cuts), ("skipped_cuts", len(pieces.skipped))]) + "\n")
        fh.write("".join("#skipped_cut\t%s\t%d\n" % sc for sc in pieces.skipped))
        fh.write("#" + "\t".join(SUMMARY_COLUMNS) + "\n")
        fh.write("".join("\t".join(r) + "\n" for r in rows))
        fh.write("#" + "\t".join(PIECE_COLUMNS) + "\n")
        for k in range(n_piece):
            a, size = int(pieces.piece_start[k]), int(pieces.sizes[k])
            cols = [pieces.names[k], names[int(pieces.parent[k])], str(a + 1), str(a + size), str(size)]
            if counters is None:
                cols += ["NA"] * 4
            else:
                cols += [str(int(counters[q, k])) for q in range(3)] + ["NA" if k in last_of_parent else str(int(spanning[k]))]
            fh.write("\t".join(cols) + "\n")
    print("SPLIT: %d cut(s) applied to %d scaffold(s), %d skipped, %d piece(s) in %s" % (n_cuts, len(pieces.applied), len(pieces.skipped),
                                                                                       n_piece, outDir))
    return pieces, rows, stats, counters


def main(argv=None, context=None):
    parser = argparse.ArgumentParser(description="Cuts scaffolds after the bases of a cuts file (supportSpans -cuts) and writes "
                                                 "every input of the pipeline for the broken assembly, the contact maps counted "
                                                 "from validPairFile on the GPU in the pieces' coordinates.")
    parser.add_argument("-config", help="Full file path to the config file", required=True, type=str)
    parser.add_argument("-cuts", help="Cuts file: scaffold <TAB> cut_after per line", required=True, type=str)
    parser.add_argument("-resolution", help="Comma-separated bin sizes in bp: one map per resolution (default: none)", type=str,
                        default=None)
    parser.add_argument("-order", help="Order file (default: finalOrderingsFile when it exists, else chromosomeOrderFile when it "
                                       "exists, else none)", type=str, default=None)
    parser.add_argument("-minPiece", help="Skip a cut closer than this to the previous kept cut or to an end (default 1)", type=int,
                        default=1)
    parser.add_argument("-out", help="Output directory (default: saveFilesDirectory/split)", type=str, default=None)
    parser.add_argument("-noBalance", help="Write the bed file and the raw map only, no ICE", action="store_true")
    parser.add_argument("-noPairs", help="Do not write split.allValidPairs", action="store_true")
    parser.add_argument("-threads", help="Host threads of the parser and the rewriter (default 0: all)", type=int, default=0)
    parser.add_argument("-device", help="GPU index (default 0)", type=int, default=0)
    args = parser.parse_args(argv)
    try:
        resolutions = parse_resolutions(args.resolution) if args.resolution is not None else []
    except ValueError as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    return runPipeline(args.config, args.cuts, resolutions, args.order, args.minPiece, args.out, balance=not args.noBalance,
                       pairs=not args.noPairs, threads=args.threads, device=args.device, context=context)


if __name__ == "__main__":
    main()
