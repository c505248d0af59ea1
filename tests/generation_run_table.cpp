// Stand-alone check of GenerationRun (kjarni_amd/csrc/generation_run.h) on the table of tests/test_generation_run_host.py: host
// code only, built with g++ -fsanitize=address,undefined by that test.  Exit status 0: every row gave its expected counts.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "generation_run.h"

using kjarni::GenerateOptions;
using kjarni::GenerationRun;
using kjarni::LastToken;

struct Case {
    const char* what;
    size_t n_prompt, capacity, max_new, max_len;
    std::vector<uint32_t> stops, defaults;
    size_t n_stream;
    long cancel_after;
    size_t emitted, asked, fed_last, fed_not_last;
};

static bool replay(const Case& c, bool feed_last, size_t* emitted, size_t* asked, size_t* fed)
{
    GenerateOptions opt;
    opt.max_new_tokens = c.max_new;
    opt.max_len = c.max_len;
    opt.stop_ids = c.stops;
    std::vector<uint32_t> out;
    GenerationRun run(std::vector<uint32_t>(c.n_prompt, 0u), opt, c.capacity, c.defaults, out);
    const std::function<bool(uint32_t)> cb = [&](uint32_t) { return c.cancel_after < 0 || (long)out.size() != c.cancel_after; };
    *asked = *fed = 0;
    while (run.wants_token() && *asked < c.n_stream)  // the stream is 100, 101, 102, ...
        if (run.accept((uint32_t)(100 + (*asked)++), cb) && run.feeds_accepted(feed_last ? LastToken::Fed : LastToken::NotFed)) ++*fed;
    *emitted = out.size();
    return run.all.size() == c.n_prompt + out.size();
}

int main()
{
    const std::vector<Case> table = {
        {"max_new_tokens = 0", 5, 20, 0, 0, {}, {}, 8, -1, 0, 0, 0, 0},
        {"a prompt already at max_len", 5, 20, 4, 5, {}, {}, 8, -1, 0, 0, 0, 0},
        {"a prompt already at the capacity", 20, 20, 4, 0, {}, {}, 8, -1, 0, 0, 0, 0},
        {"a stop id as the first token", 5, 20, 4, 0, {100}, {}, 8, -1, 0, 1, 0, 0},
        {"a stop id as the last allowed token", 5, 20, 4, 0, {103}, {}, 8, -1, 3, 4, 3, 3},
        {"a stop id one past the limit", 5, 20, 4, 0, {104}, {}, 8, -1, 4, 4, 3, 3},
        {"max_len binds before max_new_tokens", 5, 20, 8, 8, {}, {}, 8, -1, 3, 3, 2, 2},
        {"the capacity binds before both", 5, 7, 8, 12, {}, {}, 8, -1, 2, 2, 1, 1},
        {"the callback cancels at token 1", 5, 20, 4, 0, {}, {}, 8, 1, 1, 1, 0, 0},
        {"the callback cancels at the last token", 5, 20, 4, 0, {}, {}, 8, 4, 4, 4, 3, 3},
        {"an empty stop list falls back to the defaults", 5, 20, 4, 0, {}, {102}, 8, -1, 2, 3, 2, 2},
        {"an explicit stop list hides the defaults", 5, 20, 4, 0, {103}, {101}, 8, -1, 3, 4, 3, 3},
        {"a stream shorter than the run", 5, 20, 8, 0, {}, {}, 3, -1, 3, 3, 3, 3},
        {"max_len past prompt + max_new_tokens: the last token is fed where the loop says so", 5, 20, 4, 20, {}, {}, 8, -1, 4, 4, 4, 3},
        {"the default max_len is met by the last token: it is not fed", 5, 20, 4, 0, {}, {}, 8, -1, 4, 4, 3, 3},
    };
    int bad = 0;
    for (const Case& c : table)
        for (int feed_last = 0; feed_last < 2; ++feed_last) {
            size_t emitted, asked, fed;
            const bool ok = replay(c, feed_last != 0, &emitted, &asked, &fed) && emitted == c.emitted && asked == c.asked &&
                            fed == (feed_last ? c.fed_last : c.fed_not_last);
            if (!ok) {
                std::printf("FAILED %s (feed_last %d): emitted %zu asked %zu fed %zu\n", c.what, feed_last, emitted, asked, fed);
                ++bad;
            }
        }
    std::printf("%zu cases, %d failed\n", table.size(), bad);
    return bad ? 1 : 0;
}
