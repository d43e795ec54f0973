"""Record tests/golden/module_summary_*.txt: what the reference's own `print_module_summary` prints for the toy modules of
tests/test_module_summary_cpu.py (which defines them; this script imports them from there).  Run on the CPU with the reference checkout's root
as the argument; only the recorded text is committed.

    python tests/golden/make_module_summary_golden.py <reference root>
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main(reference_root):
    import test_module_summary_cpu as cases
    sys.path.insert(0, reference_root)
    from stylegan2ada.torch_utils import misc as reference_misc
    for name, (make, kwargs) in cases.CASES.items():
        module, inputs = make()
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            reference_misc.print_module_summary(module, inputs, **kwargs)
        with open(os.path.join(HERE, f"module_summary_{name}.txt"), "w") as fh:
            fh.write(text.getvalue())
        print(f"module_summary_{name}.txt: {len(text.getvalue().splitlines())} lines")


if __name__ == "__main__":
    main(sys.argv[1])
