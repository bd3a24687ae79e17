"""Rules of the library's host code that a compiler does not hold (CPU tier: reads the sources only)."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "photon_amd", "csrc")


def code_lines(path):
    for no, line in enumerate(open(path, encoding="utf-8"), 1):
        yield no, line.split("//", 1)[0]


def test_no_host_side_hipmemset():
    """hipMemset returns once its fill kernel is QUEUED on the null stream (tools/ubench/null_stream_memset.hip: 9 us, the
    fill 200 ms away behind a full chip) and a launch on a non-blocking stream is not ordered behind the null stream: a
    scene's work queues were once zeroed that way and, with eight shards side by side on one device, the fill sometimes
    ran after the march had started (groups marched twice).  Zeroing is either hipMemsetAsync on the consumer's stream
    or photon::device_zero (complete on return), or part of a host-to-device copy."""
    offenders = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        for no, code in code_lines(path):
            if re.search(r"\bhipMemset(D8|D16|D32|2D|3D)?\s*\(", code):
                offenders.append(f"{os.path.basename(path)}:{no}: {code.strip()}")
    assert not offenders, "host-asynchronous hipMemset on the null stream:\n" + "\n".join(offenders)


def test_no_host_side_device_to_device_hipmemcpy():
    """The same for hipMemcpy(..., hipMemcpyDeviceToDevice): it returns in 5 us with the copy still queued on the null
    stream, and a kernel launched afterwards on a non-blocking stream READ THE OLD BYTES in tools/ubench/null_stream_memset.hip.
    Device-to-device copies are hipMemcpyAsync on a named stream, with the wait (if any) written out."""
    offenders = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        text = "".join(code for _, code in code_lines(path))
        for m in re.finditer(r"\bhipMemcpy\s*\(([^;]*);", text):
            if "hipMemcpyDeviceToDevice" in m.group(1) or "hipMemcpyDefault" in m.group(1):
                offenders.append(f"{os.path.basename(path)}: hipMemcpy({' '.join(m.group(1).split())[:100]}")
    assert not offenders, "host-asynchronous device-to-device hipMemcpy on the null stream:\n" + "\n".join(offenders)


def _calls_outside_the_pool(names, pool=("photon_pool.hip", "photon_pool.hpp")):
    offenders = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        if os.path.basename(path) in pool:
            continue
        for no, code in code_lines(path):
            if re.search(r"\b(" + "|".join(names) + r")\s*\(", code):
                offenders.append(f"{os.path.basename(path)}:{no}: {code.strip()}")
    return offenders


def test_no_hipmalloc_or_hipfree_outside_the_pool():
    """Device memory is asked for and given back in photon_pool.hip / photon_pool.hpp alone: everywhere else a block is a
    DeviceBuffer or a PoolBuffer, released with its owner on every return path, and allocated through device_malloc, which
    empties the block cache and tries again before it reports the device out of memory."""
    offenders = _calls_outside_the_pool(["hipMalloc", "hipFree"])
    assert not offenders, "raw hipMalloc / hipFree outside photon_pool.*:\n" + "\n".join(offenders)


def test_hipmalloc_and_hipfree_are_in_photon_pool_hip_alone():
    """The header's owners release through device_free and pool_free: every block that is handed out or given back passes the
    counters of photon_selftest_alloc_stats (outstanding blocks) and the failure hook of photon_selftest_fail_alloc, which
    tests/test_alloc_failures_gpu.py relies on."""
    offenders = _calls_outside_the_pool(["hipMalloc", "hipFree"], pool=("photon_pool.hip",))
    assert not offenders, "raw hipMalloc / hipFree outside photon_pool.hip:\n" + "\n".join(offenders)


def test_no_pool_malloc_or_pool_free_outside_the_pool():
    """The same for blocks of the cache: pool_malloc and pool_free are PoolBuffer's business.  A block that somebody frees
    by hand is a block that leaks on the return path somebody forgot."""
    offenders = _calls_outside_the_pool(["pool_malloc", "pool_free"])
    assert not offenders, "pool_malloc / pool_free outside photon_pool.*:\n" + "\n".join(offenders)


ALLOCATION_SITE = r"\.alloc\(|\.reserve\(|\bscene_reserve\(|\bscene_block\(|\bdevice_malloc\("


def test_every_allocation_site_is_in_the_table_of_failed_allocations():
    """DESIGN.md section 4.3v lists, site by site, the case of tests/alloc_failure_cases.py that fails every allocation of the
    library (and the few lines the same search finds that are no device allocation).  Per source file the table's rows
    (their `n` column) add up to what the search finds: a new allocation site without a row fails here, and its row asks
    for a case."""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        n = sum(len(re.findall(ALLOCATION_SITE, code)) for _, code in code_lines(path))
        if n:
            found[os.path.basename(path)] = n
    design = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "DESIGN.md"), encoding="utf-8").read()
    section = design.split("### 4.3v ", 1)[1].split("\n### ", 1)[0]
    listed, cases = {}, set()
    for row in re.findall(r"^\| `(photon_\w+\.h(?:ip|pp))` \| ([^|]+) \| (\d+) \| ([^|]+) \|$", section, flags=re.M):
        listed[row[0]] = listed.get(row[0], 0) + int(row[2])
        cases.update(re.findall(r"`(\w+)`", row[3]))
    assert found == listed, {f: (found.get(f), listed.get(f)) for f in set(found) | set(listed) if found.get(f) != listed.get(f)}
    import alloc_failure_cases as afc
    assert cases and cases <= set(afc.CASES), sorted(cases - set(afc.CASES))


def test_the_build_knows_every_header():
    """needs_build() and the per-object staleness test look at build.HEADERS alone: a header under csrc that the list does
    not name can change without the library being rebuilt, and a GPU run then tests a stale one."""
    from photon_amd import build
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp"))}
    listed = {os.path.basename(p) for p in build.HEADERS if os.path.dirname(p) == CSRC}
    assert on_disk and on_disk == listed, sorted(on_disk ^ listed)


def test_the_window_size_rule_is_stated_once():
    """Every entry point on the (win, step) grid takes its argument rules from piv_grid.hpp: the win rule's message in a
    second file is a second statement of the rule."""
    holders = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*")))
               if "win must be 16, 32 or 64" in open(p, encoding="utf-8").read()]
    assert holders == ["piv_grid.hpp"], holders
