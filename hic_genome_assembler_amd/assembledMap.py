"""Contact maps of the assembled genome from HiC-Pro's valid pairs, on the device.

buildMap counts the read pairs on the scaffolds.  The map a scaffolding is judged by is the one of the *assembly*: the
scaffolds of a chromosome of ``finalOrderingsFile`` / ``chromosomeOrderFile`` laid end to end as Part 4 writes them -
``-`` scaffolds reversed, ``gap`` N between neighbours - and the read pairs counted in those coordinates at any bin size,
so a bin may hold the end of one scaffold, a gap and the start of the next.  Every read end is lifted on the device from
(scaffold, position) to (sequence, position) before it is binned (``hicmi_lift_maps``: one pass over ``validPairFile`` for
all resolutions), and the same pass counts the two numbers a scaffolding is summed up by: the cis / trans split per
sequence and the contact-decay histogram P(s) over cis pairs.

    python -m hic_genome_assembler_amd.assembledMap -config my_config.txt -resolution 100000,250000 \\
           [-order FILE] [-gap 100] [-chromosomesOnly] [-out DIR] [-noBalance] [-threads 0] [-device 0]

Sequences: chromosome i of the order file (1-based, file order) is ``Chr_<i>``; after the chromosomes comes every scaffold
of ``hicProScaffSizeFile`` the order file does not name, in the size file's order, as a sequence of its own under its own
name - unless ``-chromosomesOnly`` drops them (their pairs are then counted as ``unlifted``).  In ``DIR``
(``saveFilesDirectory/assembled``): ``assembly.sizes``, ``assembly.agp`` (AGP 2.0), per resolution ``res<r>/`` with the
file set buildMap writes (prefix ``assembled``) and a ``config.txt`` for ``-part1`` on the assembly's own map,
``assembled_summary.tsv``, ``assembly_stats.tsv`` and ``decay.tsv``.
"""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib
from .buildMap import MAX_BINS, STATS_COLUMNS, SUMMARY_COLUMNS, check_valid_pair_file, parse_resolutions
from .hostio import bins_from_sizes, count_bins, paused_gc, read_scaffold_sizes
from .rebinMap import output_paths, rewrite_config, scaffold_counts, write_resolution
from .writeAssembledFasta import readChromosomeOrderingFile

DEFAULT_GAP = 100                               # Part 4's nGapLength
DECAY_SLOTS = 256


@dataclass
class Assembly:
    """The sequences of an assembly and the lift of every scaffold of the size file onto them."""
    seq_names: list                 # Chr_1 .. Chr_C, then the unplaced scaffolds under their own names
    seq_sizes: np.ndarray           # int64[n_seq]
    components: list                # per sequence [(scaffold index, offset, "+" / "-"), ...] in sequence order
    n_chromosomes: int
    gap: int
    lift_seq: np.ndarray            # int32[S]  sequence of the scaffold, -1: dropped
    lift_off: np.ndarray            # int64[S]  offset of the scaffold in its sequence
    lift_rev: np.ndarray            # uint8[S]  1: reversed


def read_order_file(orderFile):
    """The chromosomes of an order file as writeAssembledFasta.readChromosomeOrderingFile reads it; ValueError for a line
    that has no orientation column."""
    try:
        return readChromosomeOrderingFile(orderFile)
    except IndexError:
        raise ValueError("order file %s has an empty line or a line without an orientation column" % orderFile)


def build_assembly(groups, names, sizes, gap=DEFAULT_GAP, chromosomes_only=False):
    """The layout of DESIGN.md 9m from the chromosomes ``groups`` ([[scaffold, orientation], ...] each) and the size file's
    (names, sizes): scaffold k of a chromosome starts at sum_{q<k} (L_q + gap).  ValueError for a scaffold the size file
    does not have, one named twice, an orientation other than + or -, an empty chromosome and a negative gap."""
    gap = int(gap)
    if gap < 0:
        raise ValueError("the gap %d is negative" % gap)
    index = {name: k for k, name in enumerate(names)}
    S = len(names)
    lift_seq = np.full(S, -1, np.int32)
    lift_off = np.zeros(S, np.int64)
    lift_rev = np.zeros(S, np.uint8)
    seq_names, seq_sizes, components = [], [], []
    for i, group in enumerate(groups, 1):
        if not group:
            raise ValueError("chromosome %d of the order file has no scaffold" % i)
        off, comps = 0, []
        for name, orientation in group:
            if name not in index:
                raise ValueError("scaffold %s of chromosome %d is not in the scaffold size file" % (name, i))
            if orientation not in ("+", "-"):
                raise ValueError("scaffold %s of chromosome %d has the orientation %r, neither + nor -" % (name, i, orientation))
            s = index[name]
            if lift_seq[s] >= 0:
                raise ValueError("scaffold %s is named twice in the order file" % name)
            if comps:
                off += gap
            lift_seq[s], lift_off[s], lift_rev[s] = i - 1, off, orientation == "-"
            comps.append((s, off, orientation))
            off += int(sizes[s])
        seq_names.append("Chr_%d" % i)
        seq_sizes.append(off)
        components.append(comps)
    n_chrom = len(seq_names)
    if not chromosomes_only:
        for s in range(S):
            if lift_seq[s] < 0:
                lift_seq[s] = len(seq_names)
                components.append([(s, 0, "+")])
                seq_names.append(names[s])
                seq_sizes.append(int(sizes[s]))
    if len(set(seq_names)) != len(seq_names):
        raise ValueError("an unplaced scaffold has the name of a chromosome (Chr_<i>)")
    return Assembly(seq_names, np.asarray(seq_sizes, np.int64), components, n_chrom, gap, lift_seq, lift_off, lift_rev)


def lift(assembly, sizes, scaf, pos):
    """(sequence, position) of the 1-based positions ``pos`` on the scaffolds ``scaf``: off + p, or off + L - p + 1 on a
    reversed scaffold; sequence -1 (and position 0) for a dropped scaffold."""
    scaf = np.asarray(scaf, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    size = np.asarray(sizes, dtype=np.int64)[scaf]
    seq = assembly.lift_seq[scaf].astype(np.int64)
    where = np.where(assembly.lift_rev[scaf] != 0, size - pos + 1, pos)
    return seq, np.where(seq >= 0, assembly.lift_off[scaf] + where, 0)


def sizes_text(assembly):
    """``assembly.sizes``: name and size of every sequence, the format of hicProScaffSizeFile."""
    return "".join("%s\t%d\n" % ns for ns in zip(assembly.seq_names, assembly.seq_sizes.tolist()))


def agp_text(assembly, names, sizes):
    """``assembly.agp`` (AGP 2.0): one W line per scaffold with its orientation, one N line per gap between neighbours
    (none for a gap of 0); an unplaced scaffold is an object of one component."""
    out = ["##agp-version\t2.0\n"]
    for seq_name, comps in zip(assembly.seq_names, assembly.components):
        part = 0
        for k, (s, off, orientation) in enumerate(comps):
            if k and assembly.gap:
                part += 1
                out.append("%s\t%d\t%d\t%d\tN\t%d\tscaffold\tyes\tproximity_ligation\n" % (
                    seq_name, off - assembly.gap + 1, off, part, assembly.gap))
            part += 1
            L = int(sizes[s])
            out.append("%s\t%d\t%d\t%d\tW\t%s\t1\t%d\t%s\n" % (seq_name, off + 1, off + L, part, names[s], L, orientation))
    return "".join(out)


def decay_slot(d):
    """Slot of the distance d in the decay histogram: 0 for d = 0, else 1 + 4 e + (((d - 2^e) * 4) >> e) with
    e = floor(log2 d) - quarter octaves in integer arithmetic."""
    d = int(d)
    if d == 0:
        return 0
    e = d.bit_length() - 1
    return 1 + 4 * e + (((d - (1 << e)) * 4) >> e)


def decay_bounds(slot):
    """(lowest, highest) distance of a slot of the decay histogram; None for a slot no distance falls in."""
    if slot == 0:
        return 0, 0
    e, q = divmod(slot - 1, 4)
    lo = (1 << e) + -(-(q << e) // 4)
    hi = (1 << e) + -(-((q + 1) << e) // 4) - 1
    return (lo, hi) if hi >= lo else None


def set_config_values(configFile, values):
    """Rewrite ``configFile`` in place with the value of every key of ``values`` replaced (rebinMap.rewrite_config); a
    key the file has no line for is added at the end, so every value holds in the written file."""
    text = rewrite_config(configFile, values)
    present = {ln.split(" = ")[0] for ln in text.splitlines() if " = " in ln and not ln.startswith("#")}
    missing = [key for key in values if key not in present]
    if missing:
        text += ("" if text.endswith("\n") or not text else "\n") + "".join("%s = %s\n" % (key, values[key]) for key in missing)
    with open(configFile, "w", newline="") as fh:
        fh.write(text)


def runPipeline(configFile, resolutions, orderFile=None, gap=DEFAULT_GAP, chromosomesOnly=False, outDir=None, balance=True,
                threads=0, device=0):
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    ice = driver.iceSettings(v)
    if outDir is None:
        outDir = os.path.join(v["saveFilesDirectory"], "assembled")
    outDir = os.path.abspath(outDir)
    if orderFile is None:
        orderFile = v["finalOrderingsFile"] if os.path.isfile(v["finalOrderingsFile"]) else v["chromosomeOrderFile"]
    try:
        check_valid_pair_file(v["validPairFile"])
        names, sizes = read_scaffold_sizes(v["hicProScaffSizeFile"])
        if not names:
            raise ValueError("hicProScaffSizeFile %s lists no scaffold" % v["hicProScaffSizeFile"])
        if not os.path.isfile(orderFile):
            raise ValueError("order file %r does not exist" % orderFile)
        asm = build_assembly(read_order_file(orderFile), names, sizes, gap, chromosomesOnly)
        for r in resolutions:
            m = count_bins(asm.seq_sizes, r)
            if m > MAX_BINS:
                raise ValueError("resolution %d needs %d bins, more than the %d a map can have" % (r, m, MAX_BINS))
    except (OSError, ValueError) as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    rows = []
    size_file = os.path.join(outDir, "assembly.sizes")
    with paused_gc():
        ctxs = [_lib.Context(device) for _r in resolutions]
        try:
            try:
                stats, (decay, cis, trans, unlifted) = _lib.lift_maps(
                    v["validPairFile"], names, sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, resolutions, ctxs,
                    threads=threads)
            except _lib.HicmiError as exc:
                sys.exit("ERROR... %s. Exiting..." % exc)
            unlifted = int(unlifted[0])
            print("ASSEMBLED: lines %d, pairs used %d, unknown scaffold %d, out of range %d, chunks %d" % stats
                  + ", unlifted %d" % unlifted)
            if stats[3]:
                print("WARNING... %d line(s) of %s have a position below 1 or beyond the size of their scaffold in %s and were "
                      "skipped: do the two files belong to one assembly?" % (stats[3], v["validPairFile"], v["hicProScaffSizeFile"]))
            os.makedirs(outDir, exist_ok=True)
            with open(size_file, "w") as fh:
                fh.write(sizes_text(asm))
            with open(os.path.join(outDir, "assembly.agp"), "w") as fh:
                fh.write(agp_text(asm, names, sizes))
            # ICE's iceMinScaffoldSize looks at the sequences, and the written configs name the assembly's own files
            v_seq = dict(v, hicProScaffSizeFile=size_file)
            further = {"hicProScaffSizeFile": size_file, "validPairFile": os.devnull, "restrictionSiteFile": os.devnull,
                       "originalFastaFile": v["assembledFastaFile"]}
            for r, ctx in zip(resolutions, ctxs):
                binList = bins_from_sizes((asm.seq_names, asm.seq_sizes), r)
                paths = output_paths(outDir, r, prefix="assembled")
                n_seq, n_one = scaffold_counts(binList)
                line = "ASSEMBLED: resolution %d, bins %d (sequences %d, of one bin %d)" % (r, len(binList), n_seq, n_one)
                ice_cols, pairs = write_resolution(ctx, binList, paths, configFile, v_seq, ice, balance, line)
                set_config_values(os.path.join(paths["dir"], "config.txt"), further)
                rows.append([str(r), str(len(binList)), str(n_seq), str(n_one)] + ice_cols + [repr(pairs)])
                ctx.close()                                             # its map is written: the memory goes back now
        finally:
            for ctx in ctxs:
                ctx.close()
    with open(os.path.join(outDir, "assembled_summary.tsv"), "w") as fh:
        fh.write("#" + "\t".join("%s=%d" % kv for kv in zip(STATS_COLUMNS + ("unlifted",), stats[:4] + (unlifted,))) + "\n")
        fh.write("#" + "\t".join(SUMMARY_COLUMNS) + "\n")
        fh.write("".join("\t".join(r) + "\n" for r in rows))

    def fraction(c, t):
        return repr(c / (c + t)) if c + t else "NA"

    total_cis, total_trans = int(cis.sum()), int(trans.sum()) // 2     # a trans pair counts in two sequences
    with open(os.path.join(outDir, "assembly_stats.tsv"), "w") as fh:
        fh.write("#sequence\tsize\tscaffolds\tcis\ttrans\tcis_fraction\n")
        for q, name in enumerate(asm.seq_names):
            c, t = int(cis[q]), int(trans[q])
            fh.write("%s\t%d\t%d\t%d\t%d\t%s\n" % (name, asm.seq_sizes[q], len(asm.components[q]), c, t, fraction(c, t)))
        fh.write("total\t%d\t%d\t%d\t%d\t%s\n" % (int(asm.seq_sizes.sum()), sum(len(c) for c in asm.components), total_cis,
                                                  total_trans, fraction(total_cis, total_trans)))
    with open(os.path.join(outDir, "decay.tsv"), "w") as fh:
        fh.write("#distance_from\tdistance_to\tpairs\n")
        for slot in np.flatnonzero(decay).tolist():
            fh.write("%d\t%d\t%d\n" % (decay_bounds(slot) + (int(decay[slot]),)))
    print("ASSEMBLED: cis %d, trans %d, cis fraction %s" % (total_cis, total_trans, fraction(total_cis, total_trans)))
    return rows, stats, (decay, cis, trans, unlifted)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Counts the contact map of the assembled genome at every resolution asked for "
                                                 "from HiC-Pro's valid pairs (validPairFile) on the GPU, with the cis / trans "
                                                 "split per sequence and the contact-decay histogram.")
    parser.add_argument("-config", help="Full file path to the config file", required=True, type=str)
    parser.add_argument("-resolution", help="Comma-separated bin sizes in bp: one output per resolution", required=True, type=str)
    parser.add_argument("-order", help="Order file (default: finalOrderingsFile when it exists, else chromosomeOrderFile)",
                        type=str, default=None)
    parser.add_argument("-gap", help="Bases between neighbouring scaffolds (default %d, as Part 4 writes)" % DEFAULT_GAP, type=int,
                        default=DEFAULT_GAP)
    parser.add_argument("-chromosomesOnly", help="Drop the scaffolds the order file does not name", action="store_true")
    parser.add_argument("-out", help="Output directory (default: saveFilesDirectory/assembled)", type=str, default=None)
    parser.add_argument("-noBalance", help="Write the bed file and the raw map only, no ICE", action="store_true")
    parser.add_argument("-threads", help="Host threads of the parser (default 0: all)", type=int, default=0)
    parser.add_argument("-device", help="GPU index (default 0)", type=int, default=0)
    args = parser.parse_args(argv)
    try:
        resolutions = parse_resolutions(args.resolution)
    except ValueError as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    runPipeline(args.config, resolutions, args.order, args.gap, args.chromosomesOnly, args.out, balance=not args.noBalance,
                threads=args.threads, device=args.device)


if __name__ == "__main__":
    main()
