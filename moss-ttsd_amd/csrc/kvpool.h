// The KV page pool: free list, per-slot page tables, owner counts and the table edits that have not reached the device.
// Pure host arithmetic, no HIP.  Only launch.h (PageEdits is set_pages_kernel's argument) and staging.h include it, and
// tests/host/pool_stage_main.cpp, which runs it on the CPU under the sanitizers.
// Invariants: a slot writes only pages that it alone owns; one shipped batch never carries a table index twice; a failed
// grow leaves no stale edit behind.  The pool launches nothing: what may have to ship a full batch takes `ship`, a
// callable int(const PageEdits&) that puts the batch on the device table (0, or the error the operation then returns).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/mtts.h"
#include "shapes.h"

struct PageEdits { int32_t n; int32_t idx[31]; int32_t val[31]; };     // page-table entries handed over as launch arguments
static_assert(sizeof(PageEdits) == 252, "PageEdits is a kernel argument: one 32-bit count + 31 (index, value) pairs");

static inline int pages_for(int tokens) { return (tokens + MTTS_PAGE - 1) / MTTS_PAGE; }

// sets the calling thread's error message, returns `code` (engine.hip defines it; the stand-alone test its own)
__attribute__((visibility("hidden"), format(printf, 2, 3))) int fail(int code, const char* fmt, ...);

class KvPool {
    int total_pages = 0, max_pages = 0, max_seq_len = 0;
    std::vector<int32_t> free_pages;
    std::vector<int32_t> h_page_table;  // [slot][max_pages]: pages a slot owns, in position order
    std::vector<int32_t> n_pages;       // pages each slot owns
    std::vector<int32_t> page_owners;   // slots whose table holds the page (> 1: a prompt page shared by takes)
    PageEdits pending_edits{};          // table entries not yet on the device

    // append `page` to the slot's table (host copy now, device copy with the next flush)
    template <typename Ship>
    int append(int slot, int page, Ship& ship) {
        const int at = slot * max_pages + n_pages[slot]++;
        h_page_table[at] = page;
        // one batch is written by the lanes of ONE store (set_pages_kernel): an index must not appear twice in it
        for (int i = 0; i < pending_edits.n; ++i)
            if (pending_edits.idx[i] == at) { pending_edits.val[i] = page; return 0; }
        if (pending_edits.n == 31)
            if (const int rc = flush(ship)) return rc;
        pending_edits.idx[pending_edits.n] = at;
        pending_edits.val[pending_edits.n++] = page;
        return 0;
    }

public:
    using Kept = std::vector<std::vector<int32_t>>;     // set_aside: the entries of the first rows
    // Free list = stack whose top is the lowest page number (a fresh pool hands pages out in ascending order); with a
    // `shuffle` seed (MTTS_PAGE_SHUFFLE, test hook) the page tables become arbitrary permutations
    void init(int total, int max_per_slot, int max_batch, int seq_len, const uint64_t* shuffle) {
        total_pages = total; max_pages = max_per_slot; max_seq_len = seq_len;
        free_pages.resize(total);
        for (int i = 0; i < total; ++i) free_pages[i] = total - 1 - i;
        if (shuffle) {
            uint64_t x = 0x9E3779B97F4A7C15ull ^ *shuffle;
            for (int i = total - 1; i > 0; --i) {
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                std::swap(free_pages[i], free_pages[(x >> 33) % (uint64_t)(i + 1)]);
            }
        }
        h_page_table.assign((size_t)max_batch * max_pages, 0);
        n_pages.assign(max_batch, 0);
        page_owners.assign(total, 0);
        pending_edits.n = 0;
    }
    int free_count() const { return (int)free_pages.size(); }
    int pages_of(int slot) const { return n_pages[slot]; }
    int32_t entry(int slot, int i) const { return h_page_table[(size_t)slot * max_pages + i]; }
    const std::vector<int32_t>& table() const { return h_page_table; }       // read-only: mtts_read_page_table, the CPU test
    const std::vector<int32_t>& counts() const { return n_pages; }
    const std::vector<int32_t>& free_list() const { return free_pages; }
    const PageEdits& pending() const { return pending_edits; }
    // table entries reach the device as one batch per ship
    template <typename Ship>
    int flush(Ship&& ship) {
        if (!pending_edits.n) return 0;
        const int rc = ship(pending_edits);
        pending_edits.n = 0;
        return rc;
    }
    // make the slot own at least `need` pages; MTTS_ENOMEM when the pool runs dry (nothing is taken back)
    template <typename Ship>
    int grow(int slot, int need, Ship&& ship) {
        if (need > max_pages) return fail(MTTS_ENOMEM, "slot %d needs %d KV pages, a sequence holds at most %d (max_seq_len %d)", slot, need, max_pages, max_seq_len);
        while (n_pages[slot] < need) {
            if (free_pages.empty()) return fail(MTTS_ENOMEM, "KV page pool exhausted (%d pages of %d tokens): slot %d needs page %d", total_pages, MTTS_PAGE, slot, n_pages[slot]);
            const int page = free_pages.back();
            free_pages.pop_back();
            page_owners[page] = 1;
            if (const int rc = append(slot, page, ship)) return rc;
        }
        return 0;
    }
    // Takes of one prompt: slot dst (empty) gets slot src's first `npages` table entries, and each of those pages one more
    // owner.  Only COMPLETE prompt pages are shared: every K/V write of a dialogue goes to a position >= its prompt
    // length, and their sealed form was made once, by the source's prefill, in the same page numbering.  (The partially
    // filled last page is copied into a private page: engine.hip, launch_fork_job.)
    template <typename Ship>
    int share(int src, int dst, int npages, Ship&& ship) {
        for (int i = 0; i < npages; ++i) {
            const int page = entry(src, i);
            page_owners[page]++;
            if (const int rc = append(dst, page, ship)) return rc;
        }
        return 0;
    }
    // every launch that could touch the slot's pages must have been issued before (stream order protects the rest:
    // the next owner's writes are enqueued after them); a page goes back on the free list with its last owner
    void release(int slot) {
        for (int i = n_pages[slot] - 1; i >= 0; --i) {
            const int page = entry(slot, i);
            if (--page_owners[page] == 0) free_pages.push_back(page);
        }
        n_pages[slot] = 0;
        // table entries of this slot that never reached the device (a grow that ended in MTTS_ENOMEM) are void now
        int k = 0;
        for (int i = 0; i < pending_edits.n; ++i)
            if (pending_edits.idx[i] / max_pages != slot) {
                pending_edits.idx[k] = pending_edits.idx[i];
                pending_edits.val[k++] = pending_edits.val[i];
            }
        pending_edits.n = k;
    }
    // a new run: every slot in ascending order, and whatever a failed run left queued
    void release_all() {
        for (int b = 0; b < (int)n_pages.size(); ++b) release(b);
        pending_edits.n = 0;
    }
    // Scoring borrows rows 0..nslots-1 while they may still list pages of an ended run: those entries are set aside (the
    // rows read as empty, the pages keep their owners) ...
    Kept set_aside(int nslots) {
        Kept kept(nslots);
        for (int b = 0; b < nslots; ++b) {
            kept[b].assign(h_page_table.begin() + (size_t)b * max_pages, h_page_table.begin() + (size_t)b * max_pages + n_pages[b]);
            n_pages[b] = 0;
        }
        return kept;
    }
    // ... and put back: the borrowed pages return to the free list in the reverse of the order they were taken in, so the
    // pool -- counts and page numbering -- is as before.  Goes through to the end; the first error is the one returned.
    template <typename Ship>
    int restore(const Kept& kept, Ship&& ship) {
        int rc = 0;
        for (int b = (int)kept.size() - 1; b >= 0; --b) release(b);
        for (int b = 0; b < (int)kept.size(); ++b)
            for (int32_t page : kept[b])
                if (const int r = append(b, page, ship)) { if (!rc) rc = r; }
        const int r = flush(ship);
        return rc ? rc : r;
    }
};
