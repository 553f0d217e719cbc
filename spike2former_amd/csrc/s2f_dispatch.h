// Runtime value -> compile-time kernel variant, for the C-ABI launchers (host side only).
//
// A launcher declares each family of kernel variants ONCE, as a constexpr table of plain structs (one entry per instance
// that is built, with a comment saying what it is for), and then writes the launch once, inside a generic lambda:
//
//   struct Tile { int cfg, MI, NJ; };
//   constexpr Tile kTiles[] = {{0, 4, 4}, {1, 2, 2}};
//   const bool ok = s2f_dispatch<kTiles>([&](const Tile& t) { return t.cfg == cfg; }, [&](auto i) {
//     constexpr Tile T = kTiles[i];
//     S2F_LAUNCH(true, true, (kernel<T.MI, T.NJ>), grid, block, 0, s, args...);
//   });
//   S2F_REQUIRE(ok, S2F_EINVAL, "...: unknown cfg %d", cfg);
//
// Only the listed entries are instantiated (the tables are deliberately subsets of the full cross product), and a value
// that matches no entry comes back as `false`: nothing is launched silently.  No heap, no std::function, no virtual
// calls: the walk is a chain of `if`s that inlines at -O3.
#pragma once
#include <stddef.h>

#include <type_traits>

template <size_t I>
using s2f_index = std::integral_constant<size_t, I>;

template <class T, size_t N>
constexpr size_t s2f_table_size(const T (&)[N]) { return N; }

// Calls f(s2f_index<I>{}) for the first I with match(TABLE[I]); false when no entry matches.
template <const auto& TABLE, size_t I = 0, class Match, class F>
static inline bool s2f_dispatch(const Match& match, const F& f) {
  if constexpr (I < s2f_table_size(TABLE)) {
    if (match(TABLE[I])) {
      f(s2f_index<I>{});
      return true;
    }
    return s2f_dispatch<TABLE, I + 1>(match, f);
  } else {
    return false;
  }
}

// The two-entry family {true, false}: f(std::true_type{}) or f(std::false_type{}).
template <class F>
static inline void s2f_dispatch_bool(bool flag, const F& f) {
  if (flag)
    f(std::true_type{});
  else
    f(std::false_type{});
}
