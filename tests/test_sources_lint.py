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


def _calls_outside_the_pool(names):
    offenders = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        if os.path.basename(path) in ("photon_pool.hip", "photon_pool.hpp"):
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


def test_no_pool_malloc_or_pool_free_outside_the_pool():
    """The same for blocks of the cache: pool_malloc and pool_free are PoolBuffer's business.  A block that somebody frees
    by hand is a block that leaks on the return path somebody forgot."""
    offenders = _calls_outside_the_pool(["pool_malloc", "pool_free"])
    assert not offenders, "pool_malloc / pool_free outside photon_pool.*:\n" + "\n".join(offenders)


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
