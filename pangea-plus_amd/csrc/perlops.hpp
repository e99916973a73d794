// Perl semantics shared by the script drop-ins (megaclust.hip, unclas.hip, trim.hip): numification of a string, truth of
// an option value, index / rindex / substr.  Host code.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <string>

namespace pgx {

inline bool p_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

// what `<`, `>` and `+=` make of a string (perlnumber): optional blanks and sign, Inf/NaN, decimal digits
// with optional fraction and exponent; anything else counts as 0, trailing text is ignored
inline double perl_num(const char *s, size_t n)
{
	size_t i = 0;
	while (i < n && p_space(s[i]))
		i++;
	const size_t st = i;
	if (i < n && (s[i] == '+' || s[i] == '-'))
		i++;
	auto low = [&](size_t k) { return k < n ? (char)tolower((unsigned char)s[k]) : '\0'; };
	if (low(i) == 'i' && low(i + 1) == 'n' && low(i + 2) == 'f')
		return s[st] == '-' ? -INFINITY : INFINITY;
	if (low(i) == 'n' && low(i + 1) == 'a' && low(i + 2) == 'n')
		return NAN;
	size_t nd = 0;
	while (i < n && isdigit((unsigned char)s[i]))
		i++, nd++;
	if (i < n && s[i] == '.') {
		i++;
		while (i < n && isdigit((unsigned char)s[i]))
			i++, nd++;
	}
	if (nd == 0)
		return 0.0;
	if (i < n && (s[i] == 'e' || s[i] == 'E')) {
		size_t j = i + 1;
		if (j < n && (s[j] == '+' || s[j] == '-'))
			j++;
		if (j < n && isdigit((unsigned char)s[j])) {
			while (j < n && isdigit((unsigned char)s[j]))
				j++;
			i = j;
		}
	}
	std::string t(s + st, i - st);
	return strtod(t.c_str(), nullptr);
}
inline double perl_num(const std::string &s) { return perl_num(s.data(), s.size()); }

// Perl truth of an option value: undef, "" and "0" are false
inline bool perl_true(const char *v) { return v && v[0] && !(v[0] == '0' && v[1] == 0); }

inline long p_index(const std::string &s, const std::string &sub, long pos)
{
	if (pos < 0)
		pos = 0;
	if ((size_t)pos > s.size())
		pos = (long)s.size();
	const size_t r = s.find(sub, (size_t)pos);
	return r == std::string::npos ? -1 : (long)r;
}
// substr(str, off, len), off >= 0; a negative len leaves that many characters off the end
inline std::string p_substr(const std::string &s, long off, long len)
{
	if (off < 0 || (size_t)off > s.size())
		return std::string();
	long end = len >= 0 ? off + len : (long)s.size() + len;
	if (end > (long)s.size())
		end = (long)s.size();
	if (end <= off)
		return std::string();
	return s.substr((size_t)off, (size_t)(end - off));
}
// rindex(str, sub, pos): the last occurrence that starts at or before pos
inline long p_rindex(const std::string &s, const std::string &sub, long pos)
{
	if (pos < 0)
		pos = 0;
	const size_t r = s.rfind(sub, (size_t)pos);
	return r == std::string::npos ? -1 : (long)r;
}
inline long p_rindex(const std::string &s, const std::string &sub) { return p_rindex(s, sub, (long)s.size()); }

} // namespace pgx
