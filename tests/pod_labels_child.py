"""Run by tests/test_pod_labels_gpu.py as a fresh process with MMP_JGROUP and / or MMP_LABEL_HASH_BITS set (the library reads the
first once per process, the second when a context is created): the whole corpus of tests/pod_labels_corpus.py against
tests/pod_labels_model.py, with that many records per wavefront / the label hashes masked to that many bits.  Prints every
difference and exits non-zero if there is one.

usage: MMP_JGROUP=3 python -m tests.pod_labels_child"""
import os
import sys

from tests.pod_labels_corpus import corpus_differences

N_BIG = 4096 + 512  # past the planted block of eight 9-element records


def main():
    diffs = corpus_differences(N_BIG)
    print("MMP_JGROUP=%s MMP_LABEL_HASH_BITS=%s: %d differences" % (os.environ.get("MMP_JGROUP"), os.environ.get("MMP_LABEL_HASH_BITS"),
                                                                    len(diffs)))
    for d in diffs:
        print(d)
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
