"""The kernel sources carry no compile-time A/B switches: a preprocessor conditional under lgteun_amd/csrc tests only the host / device
guard or one of the four stamp builds (the measuring instruments), and no `#define` is the default of an `#ifndef` of its own name.
An experiment is an edited constant in a scratch build, not a second code path parked in the product source."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / 'lgteun_amd' / 'csrc'
TEXTS = {p.name: '\n'.join(l.split('//')[0] for l in p.read_text().splitlines()) for p in CSRC.iterdir() if p.suffix in ('.hip', '.h')}
ALLOWED = {'__HIPCC__', 'LG_STAMPS', 'LG_FFT_STAMPS', 'LG_ATTN_STAMPS', 'LG_UPF_STAMPS'}


def test_conditionals_name_only_the_guard_and_the_stamp_macros():
    assert len(TEXTS) > 40
    bad = [f'{name}: {m.group(0).strip()}' for name, text in TEXTS.items() for m in re.finditer(r'^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$', text, re.M)
           if not set(re.findall(r'[A-Za-z_]\w*', m.group(1))) - {'defined'} <= ALLOWED or not re.search(r'[A-Za-z_]', m.group(1))]
    assert not bad, '\n'.join(bad)


def test_no_define_is_the_default_of_its_own_ifndef():
    bad = [f'{name}: {m.group(1)}' for name, text in TEXTS.items() for m in re.finditer(r'^[ \t]*#[ \t]*ifndef[ \t]+(\w+)\s*?\n\s*#[ \t]*define[ \t]+\1\b', text, re.M)]
    assert not bad, '\n'.join(bad)
