"""Child process of test_gpu_batch_variants.py::test_i_group_counts_other_than_the_default (not collected by pytest).

usage: batch_groups_child.py GROUPS, with MOVBA_BATCH_GROUPS=GROUPS in the environment: the library reads the variable once per
process, so every value needs a process of its own.  Runs the eight bystander windows solo and as one batch on the test
build, holds each to its solo bits and asserts the number of stream groups the batch recorded.  Exit status 0 and one line
on success; any failure is an exception."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def main():
    groups = int(sys.argv[1])
    assert os.environ.get("MOVBA_BATCH_GROUPS") == str(groups), "the library reads the group count from the environment"
    import conftest  # noqa: F401  (puts the package on sys.path)
    import test_batch_variants_cpu as cases
    import test_gpu_batch_variants as gv
    from movba import capi
    with gv.Batch(capi, cases.MONO) as b:
        b.solo()
        b.upload()
        b.run(gv.variant(1, 0, 1, groups=min(groups, 4, len(cases.MONO))))
    print(f"groups {groups}: {len(cases.MONO)} windows equal their solo bits")


if __name__ == "__main__":
    main()
