"""Shared test code lives in plain modules (batch_harness.py, kernel_harness.py, the *_numpy.py restatements), never in a test module: no
tests/test_*.py imports another test module.  A text scan of the import lines; no GPU needed."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))

#: the resource budgets: test_kernel_resources.py holds the parser of the compiler's report, and these files import it
ALLOWED = {"test_kernel_resources": {"test_cell_mlp_resources.py", "test_components_resources.py", "test_expand_resources.py", "test_extra_types_host.py",
                                     "test_hdbscan_host.py", "test_intensities_resources.py", "test_morphology_resources.py",
                                     "test_outlines_resources.py", "test_overlap_resources.py"}}

IMPORT = re.compile(r"^\s*(?:from\s+(test_\w+)\s+import\b|import\s+(test_\w+))")


def test_no_test_module_imports_another():
    offences = []
    for path in sorted(glob.glob(os.path.join(HERE, "test_*.py"))):
        name = os.path.basename(path)
        for number, line in enumerate(open(path), 1):
            m = IMPORT.match(line)
            if not m:
                continue
            module = m.group(1) or m.group(2)
            if module + ".py" == name or name in ALLOWED.get(module, ()):      # a file may name itself for a child process to import
                continue
            offences.append(f"{name}:{number}: {line.strip()}")
    assert not offences, "\n".join(offences)
