"""Case lists of the thread tests (test_kmer_thread_ref.py on the CPU, test_gpu_kmer_thread.py on the GPU): the hand-derived walks and
the generators of the random and the large cases. A case is (name, index records, k, query records); the compaction that turns
haplotypes into unitigs is the caller's (compact_ref.compact on the CPU, api.compact_unitigs on the GPU). Not a test module."""
import random

from matchtigs_amd import synth

# A Y at k = 4: the haplotypes CTTGACC + GAGTA and CTTGACC + TATCC part behind the 3-mer ACC. Stem u0 (4 windows), branch u1 (5
# windows) and branch u2 (5 windows), the latter stored as its reverse complement so that crossing into it is a step on strand -.
Y_HAPLOTYPES = ["CTTGACCGAGTA", "CTTGACCTATCC"]
Y_INDEX = ["CTTGACC", "ACCGAGTA", "GGATAGGT"]
Y_QUERIES = [
    "TTGACCGAG",     # 0: stem -> branch 1, from the stem's second window to the branch's third
    "CTCGGTCAA",     # 1: its reverse complement: the same steps reversed and flipped
    "GACCTATC",      # 2: stem -> branch 2, which is stored reversed
    "CGAGT",         # 3: starts and ends inside branch 1
    "TTGANCGAGT",    # 4: an N: five windows are not valid
    "CTTGACAGAGTA",  # 5: haplotype 0 with C -> A at 6: the four windows over it are absent
    "ACC", "",       # 6, 7: shorter than k, empty
]
#           q_record q_start q_end kmers steps first_step path_len path_start path_end
Y_WALKS = [(0, 0, 9, 6, 2, 0, 12, 1, 10),
           (1, 0, 9, 6, 2, 2, 12, 2, 11),
           (2, 0, 8, 5, 2, 4, 12, 3, 11),
           (3, 0, 5, 2, 1, 6, 8, 2, 7),
           (4, 0, 4, 1, 1, 7, 7, 1, 5), (4, 5, 10, 2, 1, 8, 8, 2, 7),
           (5, 0, 6, 3, 1, 9, 7, 0, 6), (5, 7, 12, 2, 1, 10, 8, 3, 8)]
Y_STEPS = [0, 2,  3, 1,  0, 5,  2,  0, 2,  0, 2]  # (u << 1) | strand
Y_COUNTS = {"kmers": [6, 6, 5, 2, 7, 9, 0, 0], "valid": [6, 6, 5, 2, 3, 9, 0, 0], "found": [6, 6, 5, 2, 3, 5, 0, 0]}
Y_GAF = (b"r0\t9\t0\t9\t+\t>0>1\t12\t1\t10\t9\t9\t255\tcg:Z:9=\tkm:i:6\n"
         b"r1\t9\t0\t9\t+\t<1<0\t12\t2\t11\t9\t9\t255\tcg:Z:9=\tkm:i:6\n"
         b"r2\t8\t0\t8\t+\t>0<2\t12\t3\t11\t8\t8\t255\tcg:Z:8=\tkm:i:5\n"
         b"r3\t5\t0\t5\t+\t>1\t8\t2\t7\t5\t5\t255\tcg:Z:5=\tkm:i:2\n"
         b"r4\t10\t0\t4\t+\t>0\t7\t1\t5\t4\t4\t255\tcg:Z:4=\tkm:i:1\n"
         b"r4\t10\t5\t10\t+\t>1\t8\t2\t7\t5\t5\t255\tcg:Z:5=\tkm:i:2\n"
         b"r5\t12\t0\t6\t+\t>0\t7\t0\t6\t6\t6\t255\tcg:Z:6=\tkm:i:3\n"
         b"r5\t12\t7\t12\t+\t>1\t8\t3\t8\t5\t5\t255\tcg:Z:5=\tkm:i:2\n")
# The ring AACTG at k = 4, cut open at its first base: five windows. The read enters at the third window and goes round twice more.
RING_INDEX = ["AACTGAAC"]
RING_QUERIES = ["CTGAACTGAACTGAAC", "GTTCAGTTCAG"]  # (the second: backwards from the ring's last window, one full turn and three windows)
RING_WALKS = [(0, 0, 16, 13, 3, 0, 18, 2, 18), (1, 0, 11, 8, 2, 3, 13, 0, 11)]
RING_STEPS = [0, 0, 0, 1, 1]


def hand_cases():
    return [("Y", Y_INDEX, 4, Y_QUERIES, {**Y_COUNTS, "walks": Y_WALKS, "steps": Y_STEPS}),
            ("ring", RING_INDEX, 4, RING_QUERIES, {"kmers": [13, 8], "valid": [13, 8], "found": [13, 8], "walks": RING_WALKS, "steps": RING_STEPS})]


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def reads_of(rng, haps, k, n_reads, max_len):
    """Pieces of the haplotypes from both strands, some with substitutions and Ns, then the awkward records."""
    out = []
    for _ in range(n_reads):
        h = rng.choice(haps)
        n = rng.randint(max(1, k - 2), max_len)
        at = rng.randrange(0, len(h) - n)
        s = h[at:at + n]
        s = list(synth.revcomp(s) if rng.random() < 0.5 else s)
        if rng.random() < 0.6:
            for j in range(len(s)):
                if rng.random() < 0.02:
                    s[j] = rng.choice("ACGTNn")
        out.append("".join(s) if rng.random() < 0.8 else "".join(s).lower())
    return out + ["", "A" * (k - 1), "N" * (k + 3)]


def genome_case(k, seed=36):
    """Two haplotypes of 2 kb that differ in SNPs, and reads of them: -> (haplotypes, queries); the haplotypes themselves, forwards
    and backwards, are queries too (one walk each over their own unitigs)."""
    rng = random.Random(1000 * seed + k)
    haps = synth.random_genome(2000, seed=seed + k, haplotypes=2, sub_rate=0.02)
    return haps, [haps[0], synth.revcomp(haps[1])] + reads_of(rng, haps, k, 40, 300)


def large_case(seed=5):
    """k = 5 over a genome of 20 kb, which holds every 5-mer (asserted by the tests): whatever ACGT string is asked is found window by
    window, over unitigs of one or two windows. One record of 100 kb is one walk of tens of thousands of steps; 3 000 short reads
    with an N each make thousands of walks: runs and walks both span several tiles of hu::scan_u32 (2 048 items)."""
    rng = random.Random(seed)
    genome = [dna(rng, 20_000)]
    long_record = dna(rng, 100_000)
    reads = []
    for _ in range(3000):
        s = list(dna(rng, rng.randint(20, 45)))
        s[rng.randrange(len(s))] = "N"
        reads.append("".join(s))
    return genome, 5, reads[:1500] + [long_record] + reads[1500:]
